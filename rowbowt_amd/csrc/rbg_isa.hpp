// rbg_isa.hpp -- the ISA sample: from a text position p the row of the suffix at p, through sampled pairs {text position, row} and a walk by FL (rbg_fl.hpp).
// Host and device share this text; a host compiler takes it alone (tests/cpp/isa_check.cpp drives builder and lookup against a naive ISA).
// rbg_extract_prepare (capi/extract.ipp) builds it from the handle's run arrays and toehold samples, extract.hip walks from it.
//
// SAMPLES.  Pairs {tpos, row} with tpos = SA[row], from two sources.  (1) Every run i of the BWT gives its last row: row = run_start[i + 1] - 1, tpos =
// (samples_last[i] + 1) mod n (the toehold keeps SA - 1 there).  (2) Every row whose BWT symbol is not one of A C G T and which is not the last of its run
// gives a pair too: its SA comes from the run's last row downwards by the host's phi rule over pred_pos / phi_base (phi(SA[row]) = SA[row - 1]), one phi
// step per such row.  The second group makes the walk total: if T[s] is no base, the suffix at s + 1 has a non-base BWT symbol, so s + 1 is a sample -- no
// non-base byte lies between a position and the sample before it, and FL (which has no answer on a non-base row) is never asked there.  Position 0 is always
// a sample: its BWT symbol is the terminator, a run of one.  Text positions are distinct; the samples are stored sorted by tpos as entries {tpos, row} side
// by side (2 x 4 bytes at 4-byte positions, else 2 x 8), so one load brings both.
//
// DIRECTORY over TEXT POSITION, the shape of FL's over rank: dir[b] = the index of the largest sample with tpos <= b << shift, shift = max(0, floor(log2(n /
// S))), (n >> shift) + 2 entries of the position width.  The sample before p lies in [dir[b], dir[b + 1]] for b = p >> shift: a bounded bisection.
//
// LOOKUP.  isa_lookup(p) = the sample {q, row_q} with the largest q <= p; the row of p is p - q FL steps from row_q.
//
// BYTES.  S * 2 * pos_bytes + ((n >> shift) + 2) * pos_bytes; S is r plus the non-base rows that do not end a run.
#ifndef RBG_ISA_HPP
#define RBG_ISA_HPP
#include "rbg_fl.hpp"

#include <algorithm>

namespace rbg {

template <typename P>
struct alignas(2 * sizeof(P)) IsaEnt {
    P tpos, row;
};
static_assert(sizeof(IsaEnt<uint32_t>) == 8 && sizeof(IsaEnt<uint64_t>) == 16, "one load brings tpos and row");

// the structure as a walk sees it
struct IsaView {
    const void *ent;      // IsaEnt<P>[samples], ascending tpos, ent[0].tpos == 0
    const void *dir;      // P[(n >> shift) + 2]
    uint64_t n, samples;
    uint32_t shift;
};

struct IsaHit {
    uint64_t tpos, row;
};

RBG_FL_HD bool isa_is_base(const uint32_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

// the sample before p (p < n).  probes (nullable): entries fetched by the bisection
template <typename P>
RBG_FL_HD IsaHit isa_lookup(const IsaView &v, const uint64_t p, unsigned long long *probes = nullptr) {
    const IsaEnt<P> *__restrict__ ent = static_cast<const IsaEnt<P> *>(v.ent);
    const P *__restrict__ dir = static_cast<const P *>(v.dir);
    const uint64_t b = p >> v.shift;
    uint64_t a = dir[b], z = dir[b + 1];          // tpos[a] <= p; the answer lies in [a, z]
    while (a < z) {
        const uint64_t mid = a + ((z - a + 1) >> 1);
        if (probes) *probes += 1;
        if (static_cast<uint64_t>(ent[mid].tpos) <= p) a = mid; else z = mid - 1;
    }
    const IsaEnt<P> e = ent[a];
    return IsaHit{static_cast<uint64_t>(e.tpos), static_cast<uint64_t>(e.row)};
}

// the row of the suffix at p: the lookup, then p - q FL steps.  kFlNone when a row on the way has no base (never on an index built from a BWT: see SAMPLES)
template <typename P>
RBG_FL_HD uint64_t isa_row(const IsaView &v, const FlView &fl, const uint64_t p) {
    const IsaHit h = isa_lookup<P>(v, p);
    uint64_t row = h.row;
    for (uint64_t d = p - h.tpos; d; --d) {
        const FlStep st = fl_step<P>(fl, row);
        if (!st.sym) return kFlNone;
        row = st.next;
    }
    return row;
}

// ---- the host side -------------------------------------------------------------------------------------------------------------------------
inline uint32_t isa_shift(const uint64_t n, const uint64_t samples) { return fl_shift(n, samples); }
inline uint64_t isa_dir_entries(const uint64_t n, const uint32_t shift) { return (n >> shift) + 2; }
inline uint64_t isa_bytes(const uint64_t n, const uint64_t samples, const uint32_t pos_bytes) {
    return samples * 2 * pos_bytes + isa_dir_entries(n, isa_shift(n, samples)) * pos_bytes;
}

struct IsaIndex {
    uint32_t pos_bytes = 0, shift = 0;
    uint64_t n = 0, samples = 0, dir_entries = 0;
    uint64_t second_kind = 0;      // samples of non-base rows that do not end a run
    uint64_t max_gap = 0;          // the largest tpos[j + 1] - tpos[j], n closing the list: a walk-in takes fewer steps than this
    std::vector<unsigned char> blob;      // ONE block: the entries, then the directory
    uint64_t dir_at = 0;           // byte offset of the directory in blob
    uint64_t bytes() const { return blob.size(); }
    IsaView view(const void *base) const {
        return IsaView{base, static_cast<const unsigned char *>(base) + dir_at, n, samples, shift};
    }
};

struct IsaPair {
    uint64_t tpos, row;
};

// the host's phi over the sorted run-start samples (toehold_sa.hpp:56-72): pred_pos[j] = SA[first row of a run] - 1 ascending, phi_base[j] = SA - 1 at the
// last row of the run before it.  i = SA[row], row >= 1 -> SA[row - 1]
inline uint64_t isa_phi(const uint64_t *pred_pos, const uint64_t *phi_base, const uint64_t R, const uint64_t n, const uint64_t i) {
    const uint64_t below = static_cast<uint64_t>(std::lower_bound(pred_pos, pred_pos + R, i) - pred_pos);      // samples < i
    const uint64_t jr = below ? below - 1 : R - 1;
    const uint64_t j = pred_pos[jr];
    const uint64_t delta = j < i ? i - j : i + 1;
    return (phi_base[jr] + delta) % n;
}

// every pair, unsorted: the runs' last rows, then the non-base rows above them
inline void isa_collect(const uint8_t *heads, const uint64_t *run_start, const uint64_t R, const uint64_t *samples_last, const uint64_t *pred_pos,
                        const uint64_t *phi_base, const uint64_t n, std::vector<IsaPair> &out, uint64_t &second_kind) {
    out.clear();
    second_kind = 0;
    for (uint64_t g = 0; g < R; ++g)
        if (!isa_is_base(heads[g])) second_kind += run_start[g + 1] - run_start[g] - 1;
    out.reserve(R + second_kind);
    for (uint64_t g = 0; g < R; ++g) out.push_back(IsaPair{(samples_last[g] + 1) % n, run_start[g + 1] - 1});
    for (uint64_t g = 0; g < R; ++g) {
        if (isa_is_base(heads[g])) continue;
        uint64_t sa = (samples_last[g] + 1) % n;
        for (uint64_t row = run_start[g + 1] - 1; row > run_start[g]; --row) {
            sa = isa_phi(pred_pos, phi_base, R, n, sa);
            out.push_back(IsaPair{sa, row - 1});
        }
    }
}

// ascending tpos: an LSD radix sort, 11 bits a pass over the bits n has (a comparison sort of 4e7 pairs takes seconds)
inline void isa_sort(std::vector<IsaPair> &v, const uint64_t n) {
    int bits = 1;
    while (bits < 64 && (n >> bits)) ++bits;
    constexpr int kDigit = 11;
    constexpr size_t kBuckets = size_t(1) << kDigit;
    std::vector<IsaPair> w(v.size());
    std::vector<uint64_t> hist(kBuckets);
    for (int shift = 0; shift < bits; shift += kDigit) {
        std::fill(hist.begin(), hist.end(), 0);
        for (const IsaPair &e : v) ++hist[(e.tpos >> shift) & (kBuckets - 1)];
        uint64_t sum = 0;
        for (uint64_t &h : hist) { const uint64_t c = h; h = sum; sum += c; }
        for (const IsaPair &e : v) w[hist[(e.tpos >> shift) & (kBuckets - 1)]++] = e;
        v.swap(w);
    }
}

template <typename P>
inline void isa_fill(const std::vector<IsaPair> &s, IsaIndex &out) {
    IsaEnt<P> *ent = reinterpret_cast<IsaEnt<P> *>(out.blob.data());
    P *dir = reinterpret_cast<P *>(out.blob.data() + out.dir_at);
    uint64_t nextb = 0;      // the next bucket to fill
    for (uint64_t j = 0; j < s.size(); ++j) {
        ent[j] = IsaEnt<P>{static_cast<P>(s[j].tpos), static_cast<P>(s[j].row)};
        // every bucket whose first position lies before the next sample's has this sample before it
        const uint64_t upto = j + 1 < s.size() ? s[j + 1].tpos : ~uint64_t(0);
        while (nextb < out.dir_entries && (nextb << out.shift) < upto) dir[nextb++] = static_cast<P>(j);
    }
}

// from pairs already collected (sorted here).  false: pos_bytes is neither 4 nor 8, or 4 with n >= 2^32, no sample at position 0, a position or a row >= n,
// or two samples at one position
inline bool isa_build_pairs(std::vector<IsaPair> &s, const uint64_t n, const uint32_t pos_bytes, const uint64_t second_kind, IsaIndex &out) {
    out = IsaIndex();
    if ((pos_bytes != 4 && pos_bytes != 8) || n == 0 || s.empty()) return false;
    if (pos_bytes == 4 && (n >> 32)) return false;
    for (const IsaPair &e : s)
        if (e.tpos >= n || e.row >= n) return false;
    isa_sort(s, n);
    if (s[0].tpos != 0) return false;
    out.pos_bytes = pos_bytes;
    out.n = n;
    out.samples = s.size();
    out.second_kind = second_kind;
    for (uint64_t j = 0; j < s.size(); ++j) {
        const uint64_t next = j + 1 < s.size() ? s[j + 1].tpos : n;
        if (next <= s[j].tpos) return false;
        out.max_gap = std::max(out.max_gap, next - s[j].tpos);
    }
    out.shift = isa_shift(n, out.samples);
    out.dir_entries = isa_dir_entries(n, out.shift);
    out.dir_at = out.samples * 2 * pos_bytes;
    out.blob.assign(out.dir_at + out.dir_entries * pos_bytes, 0);
    if (pos_bytes == 4) isa_fill<uint32_t>(s, out); else isa_fill<uint64_t>(s, out);
    return true;
}

// heads[R], run_start[R + 1] (run_start[R] = n), samples_last[R] (BWT-run order), pred_pos[R] / phi_base[R] (text order): HostIndex's arrays
inline bool isa_build(const uint8_t *heads, const uint64_t *run_start, const uint64_t R, const uint64_t *samples_last, const uint64_t *pred_pos,
                      const uint64_t *phi_base, const uint32_t pos_bytes, IsaIndex &out) {
    out = IsaIndex();
    if (!R) return false;
    const uint64_t n = run_start[R];
    for (uint64_t g = 0; g < R; ++g)
        if (run_start[g + 1] <= run_start[g] || samples_last[g] >= n || pred_pos[g] >= n || phi_base[g] >= n) return false;
    std::vector<IsaPair> s;
    uint64_t second = 0;
    isa_collect(heads, run_start, R, samples_last, pred_pos, phi_base, n, s, second);
    return isa_build_pairs(s, n, pos_bytes, second, out);
}

}  // namespace rbg
#endif
