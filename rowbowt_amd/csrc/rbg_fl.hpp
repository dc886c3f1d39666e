// rbg_fl.hpp -- the FL index: FL(i) = select_c(BWT, i - F[c]), the inverse of LF, over the runs of the BWT.  From the row of the suffix at text position p it
// gives T[p] (the row's F symbol c) and the row of the suffix at p + 1.  Host and device share this text; a host compiler takes it alone
// (tests/cpp/fl_check.cpp drives builder and step against a select over the expanded BWT).  rbg_fl_prepare (capi/fl.ipp) builds it from the handle's
// run heads and run starts, fl_extend.hip walks it.
//
// RUN ENTRIES.  Per base c of A C G T that the BWT holds, the c-runs in BWT order, one entry {cum, pos} each: cum = the number of c before the run,
// pos = the BWT position where it starts; cum and pos side by side (2 x 4 bytes at 4-byte positions, else 2 x 8), so one load brings both.  A closing
// sentinel {n_c, n} follows the runs_c entries.
//
// DIRECTORY.  Per base, over RANK: dir[k >> shift] = the index of the run that holds rank (k >> shift) << shift -- the largest j with cum[j] <= that
// rank, which is the sentinel's index runs_c for a rank >= n_c.  shift = max(0, floor(log2(n_c / runs_c))): the largest s with runs_c << s <= n_c, so the
// directory has about as many entries as the run list, (n_c >> shift) + 2 of them (the bucket of every rank and the one behind it).  A bucket covers 2^shift
// ranks and every run has at least one symbol, so dir[b + 1] - dir[b] <= 2^shift: the run of rank k lies in [dir[b], dir[b + 1]], a bounded bisection.
//
// STEP.  fl_step(row): c = the base with F[c] <= row < F[c] + n_c (none: "no base" -- the row of a terminator, a separator, an N, anything else; the
// walk ends there as the left walk ends on such a byte); k = row - F[c]; b = k >> shift; the run j of rank k within [dir[b], dir[b + 1]]; the answer is
// {c, pos[j] + (k - cum[j])}.  The common bucket costs two dependent fetches: the directory pair, then entries dir[b] and dir[b] + 1 (the second always
// exists: the sentinel).  Only when the run is neither of them is [dir[b] + 2, dir[b + 1]] searched.
//
// BYTES.  Per base (runs_c + 1) * 2 * pos_bytes + ((n_c >> shift) + 2) * pos_bytes (directory entries have the position width: a run index is below n);
// fl_bytes() sums it.  Everything is proportional to r.
#ifndef RBG_FL_HPP
#define RBG_FL_HPP
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RBG_FL_HD __host__ __device__ __forceinline__
#else
#define RBG_FL_HD inline
#endif

#include <cstdint>
#include <cstring>
#include <vector>

namespace rbg {

constexpr uint32_t kFlBases = 4;
constexpr uint64_t kFlNone = ~uint64_t(0);     // FL of a row that has no base
RBG_FL_HD uint32_t fl_base_byte(const uint32_t j) { return j == 0 ? 'A' : j == 1 ? 'C' : j == 2 ? 'G' : 'T'; }

template <typename P>
struct alignas(2 * sizeof(P)) FlEnt {
    P cum, pos;
};
static_assert(sizeof(FlEnt<uint32_t>) == 8 && sizeof(FlEnt<uint64_t>) == 16, "one load brings cum and pos");

// the structure as a walk sees it, base j = A C G T (a base the BWT lacks: total = 0, nothing else read)
struct FlView {
    const void *ent[kFlBases];     // FlEnt<P>[runs + 1]
    const void *dir[kFlBases];     // P[(total >> shift) + 2]
    uint64_t F[kFlBases], total[kFlBases];
    uint32_t shift[kFlBases];
};

struct FlStep {
    uint32_t sym;      // the row's F byte when it is one of A C G T, else 0
    uint64_t next;     // FL(row), or kFlNone
};

inline uint32_t fl_shift(const uint64_t total, const uint64_t runs) {
    uint32_t s = 0;
    while (s < 63 && runs && ((runs << (s + 1)) >> (s + 1)) == runs && (runs << (s + 1)) <= total) ++s;
    return s;
}
inline uint64_t fl_dir_entries(const uint64_t total, const uint32_t shift) { return (total >> shift) + 2; }
inline uint64_t fl_base_bytes(const uint64_t total, const uint64_t runs, const uint32_t pos_bytes) {
    return runs ? (runs + 1) * 2 * pos_bytes + fl_dir_entries(total, fl_shift(total, runs)) * pos_bytes : 0;
}

// the run of rank k (k < total of its base): the largest j with cum[j] <= k.  probes (nullable): entries fetched beyond the first pair
template <typename P>
RBG_FL_HD uint64_t fl_select(const FlEnt<P> *__restrict__ ent, const P *__restrict__ dir, const uint32_t shift, const uint64_t k,
                             unsigned long long *probes = nullptr) {
    const uint64_t b = k >> shift;
    const uint64_t lo = dir[b], hi = dir[b + 1];
    const FlEnt<P> e0 = ent[lo], e1 = ent[lo + 1];
    if (static_cast<uint64_t>(e1.cum) > k) return static_cast<uint64_t>(e0.pos) + (k - e0.cum);
    if (hi <= lo + 1) return static_cast<uint64_t>(e1.pos) + (k - e1.cum);
    uint64_t a = lo + 1, z = hi;          // cum[a] <= k; the answer lies in [a, z]
    while (a < z) {
        const uint64_t mid = a + ((z - a + 1) >> 1);
        if (probes) *probes += 1;
        if (static_cast<uint64_t>(ent[mid].cum) <= k) a = mid; else z = mid - 1;
    }
    if (probes) *probes += 1;
    const FlEnt<P> e = ent[a];
    return static_cast<uint64_t>(e.pos) + (k - e.cum);
}

template <typename P>
RBG_FL_HD FlStep fl_step(const FlView &v, const uint64_t row, unsigned long long *probes = nullptr) {
    uint32_t j = kFlBases;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t c = 0; c < kFlBases; ++c)
        if (row - v.F[c] < v.total[c]) j = c;      // (row below F[c] wraps to a huge value; the bases' intervals are disjoint)
    if (j == kFlBases) return FlStep{0u, kFlNone};
    const uint64_t next = fl_select<P>(static_cast<const FlEnt<P> *>(v.ent[j]), static_cast<const P *>(v.dir[j]), v.shift[j], row - v.F[j], probes);
    return FlStep{fl_base_byte(j), next};
}

// ---- the host side -------------------------------------------------------------------------------------------------------------------------
struct FlIndex {
    uint32_t pos_bytes = 0;
    uint64_t n = 0;
    uint64_t F[kFlBases] = {}, total[kFlBases] = {}, runs[kFlBases] = {}, dir_entries[kFlBases] = {};
    uint32_t shift[kFlBases] = {};
    // ONE block: the four run lists back to back, then the four directories (each list a multiple of the entry's size: nothing is padded)
    std::vector<unsigned char> blob;
    uint64_t ent_at[kFlBases] = {}, dir_at[kFlBases] = {};      // byte offsets into blob
    uint64_t bytes() const { return blob.size(); }
    FlView view(const void *base) const {
        FlView v;
        for (uint32_t j = 0; j < kFlBases; ++j) {
            v.ent[j] = static_cast<const unsigned char *>(base) + ent_at[j];
            v.dir[j] = static_cast<const unsigned char *>(base) + dir_at[j];
            v.F[j] = F[j]; v.total[j] = total[j]; v.shift[j] = shift[j];
        }
        return v;
    }
};

template <typename P>
inline void fl_fill(const uint8_t *heads, const uint64_t *run_start, const uint64_t R, FlIndex &out) {
    FlEnt<P> *ent[kFlBases];
    P *dir[kFlBases];
    uint64_t at[kFlBases] = {}, cum[kFlBases] = {}, nextb[kFlBases] = {};      // entries written, symbols seen, the next bucket to fill
    for (uint32_t j = 0; j < kFlBases; ++j) {
        ent[j] = reinterpret_cast<FlEnt<P> *>(out.blob.data() + out.ent_at[j]);
        dir[j] = reinterpret_cast<P *>(out.blob.data() + out.dir_at[j]);
    }
    auto fill_dir = [&](const uint32_t j, const uint64_t upto_rank, const uint64_t run) {      // every bucket whose first rank is < upto_rank starts in `run`
        while (nextb[j] < out.dir_entries[j] && (nextb[j] << out.shift[j]) < upto_rank) dir[j][nextb[j]++] = static_cast<P>(run);
    };
    for (uint64_t g = 0; g < R; ++g) {
        uint32_t j = kFlBases;
        for (uint32_t c = 0; c < kFlBases; ++c)
            if (heads[g] == fl_base_byte(c)) j = c;
        if (j == kFlBases) continue;
        const uint64_t len = run_start[g + 1] - run_start[g];
        ent[j][at[j]] = FlEnt<P>{static_cast<P>(cum[j]), static_cast<P>(run_start[g])};
        fill_dir(j, cum[j] + len, at[j]);
        cum[j] += len;
        at[j] += 1;
    }
    for (uint32_t j = 0; j < kFlBases; ++j) {
        if (!out.runs[j]) continue;
        ent[j][at[j]] = FlEnt<P>{static_cast<P>(out.total[j]), static_cast<P>(out.n)};
        while (nextb[j] < out.dir_entries[j]) dir[j][nextb[j]++] = static_cast<P>(out.runs[j]);      // ranks >= n_c: the sentinel
    }
}

// heads[R], run_start[R + 1] (run_start[R] = n), F[256] = the symbols smaller than each byte (rbg_get_f's values).  false: pos_bytes is neither 4 nor 8,
// or 4 with n >= 2^32, or the runs do not ascend
inline bool fl_build(const uint8_t *heads, const uint64_t *run_start, const uint64_t R, const uint64_t *F, const uint32_t pos_bytes, FlIndex &out) {
    out = FlIndex();
    if (pos_bytes != 4 && pos_bytes != 8) return false;
    out.pos_bytes = pos_bytes;
    out.n = R ? run_start[R] : 0;
    if (pos_bytes == 4 && (out.n >> 32)) return false;
    for (uint64_t g = 0; g < R; ++g) {
        if (run_start[g + 1] <= run_start[g]) return false;
        for (uint32_t c = 0; c < kFlBases; ++c)
            if (heads[g] == fl_base_byte(c)) { out.runs[c] += 1; out.total[c] += run_start[g + 1] - run_start[g]; }
    }
    uint64_t at = 0;
    for (uint32_t j = 0; j < kFlBases; ++j) {
        out.F[j] = F[fl_base_byte(j)];
        out.shift[j] = fl_shift(out.total[j], out.runs[j]);
        out.dir_entries[j] = out.runs[j] ? fl_dir_entries(out.total[j], out.shift[j]) : 0;
        out.ent_at[j] = at;
        at += out.runs[j] ? (out.runs[j] + 1) * 2 * pos_bytes : 0;
    }
    for (uint32_t j = 0; j < kFlBases; ++j) {
        out.dir_at[j] = at;
        at += out.dir_entries[j] * pos_bytes;
    }
    out.blob.assign(at, 0);
    if (pos_bytes == 4) fl_fill<uint32_t>(heads, run_start, R, out); else fl_fill<uint64_t>(heads, run_start, R, out);
    return true;
}

}  // namespace rbg
#endif
