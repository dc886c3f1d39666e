// k_tally.hip -- the marker tally (rbg_tally_*, rbg_markers_tally; include/rbg.h): per marker, how many printed lines of rb_markers carried it.
//
//   k_tally_add          one lane per marker element of the records k_report_select left (the element -> record map of the text path:
//                        launch_report_melem / launch_report_map), into the table
//   k_tally_add_reads    the same elements in per-read mode: of a read's lines that carry a marker one line counts; optionally, a read with two
//                        alleles of a site counts for neither (see "per-read mode" below)
//   k_tally_add_entries  host-provided entries (another tally's export) into the table: the merge
//   k_tally_rehash       every live slot of an old table into a new one (the grow)
//   k_tally_live/gather  count, scan and gather the live slots into a dense rbg_tally_entry_t array (the export; sorted on the host)
//
// THE TABLE.  Open addressing with linear probing over `cap` (a power of two) slots of 32 bytes {key, n_fwd, n_rev, len_sum}: one slot is one
// 32-byte sector.  The empty key is 2^64 - 1; the MARKER 2^64 - 1 has a slot of its own in the header, so every 64-bit value is a legal key.
// A slot is claimed by a 64-bit compare-and-swap on its key and then only ever added to (three 64-bit atomic adds): sums of integers, so the
// table's content as a set of entries does not depend on the order in which lanes, waves, passes or calls arrive (WHERE a key sits does).
// Header (8 u64): [0] -, [1..3] the sums of marker 2^64 - 1, [4] dropped, [5] claimed slots, [6] records added, [7] elements added.
//
// THE BOUND.  A probe sequence visits at most `cap` slots; an element that finds neither its key nor an empty slot is counted in `dropped` and
// left out.  The host keeps the load factor at or below 1/2 (capi/tally.ipp: nothing is launched without reserved room), so the bound is a
// backstop: no launch can spin on a full table.
//
// COMBINING.  Before going to memory the lanes of a wave that hold the same key combine: a ballot / broadcast loop over the distinct keys of the
// wave, the first lane of each group adds the group's sums.  Reads of neighbouring text positions share markers, so a coordinate-sorted batch
// puts equal keys into one wave.  COMBINE = false (RBG_TALLY_COMBINE=0) sends every lane's own addition: the same table content.
#include <hipcub/hipcub.hpp>

#include "../../include/rbg.h"
#include "rbg_dev.h"

namespace rbg {
namespace {

constexpr uint64_t kTallyEmpty = ~uint64_t(0);
typedef unsigned long long ull;

struct TallyTab {
    uint64_t *slots;   // cap slots of four u64
    uint64_t cap;      // a power of two
    uint64_t *hdr;     // eight u64 (see above)
};

__device__ __forceinline__ uint64_t tally_mix(uint64_t x) {   // the 64-bit finaliser of MurmurHash3: every input bit reaches every output bit
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}

__device__ __forceinline__ void tally_sums(uint64_t *s, const uint64_t nf, const uint64_t nr, const uint64_t ls) {
    if (nf) atomicAdd(reinterpret_cast<ull *>(s + 1), static_cast<ull>(nf));
    if (nr) atomicAdd(reinterpret_cast<ull *>(s + 2), static_cast<ull>(nr));
    if (ls) atomicAdd(reinterpret_cast<ull *>(s + 3), static_cast<ull>(ls));
}

// key's slot gets the three sums; at most cap probes
__device__ __forceinline__ void tally_insert(const TallyTab &t, const uint64_t key, const uint64_t nf, const uint64_t nr, const uint64_t ls) {
    if (key == kTallyEmpty) {
        tally_sums(t.hdr, nf, nr, ls);
        return;
    }
    const uint64_t mask = t.cap - 1;
    uint64_t h = tally_mix(key) & mask;
    for (uint64_t probe = 0; probe < t.cap; ++probe, h = (h + 1) & mask) {
        uint64_t *const s = t.slots + 4 * h;
        uint64_t k = __atomic_load_n(s, __ATOMIC_RELAXED);
        if (k == kTallyEmpty) {
            k = atomicCAS(reinterpret_cast<ull *>(s), static_cast<ull>(kTallyEmpty), static_cast<ull>(key));
            if (k == kTallyEmpty) {
                atomicAdd(reinterpret_cast<ull *>(t.hdr + 5), ull(1));
                k = key;
            }
        }
        if (k == key) {
            tally_sums(s, nf, nr, ls);
            return;
        }
    }
    atomicAdd(reinterpret_cast<ull *>(t.hdr + 4), ull(1));
}

// One addition per lane (key: +1 to n_fwd or n_rev by `rev`, +qlen to len_sum) where `active`; every lane of the wave calls it.  COMBINE: the lanes
// that hold the same key combine first (see the head of the file), the first lane of each group adds the group's sums.
template <bool COMBINE>
__device__ __forceinline__ void tally_wave_add(const TallyTab &t, const bool active, const uint64_t key, const bool rev, const uint64_t qlen) {
    if (!COMBINE) {
        if (active) tally_insert(t, key, rev ? 0 : 1, rev ? 1 : 0, qlen);
        return;
    }
    const int lane = threadIdx.x & 63;
    uint64_t todo = __ballot(active);
    uint64_t nf = 0, nr = 0, ls = 0;
    bool lead = false;
    while (todo) {   // one turn per distinct key of the wave
        const int l = __ffsll(static_cast<long long>(todo)) - 1;
        const uint64_t k = __shfl(key, l);
        const bool same = active && key == k;
        const uint64_t m = __ballot(same), mr = __ballot(same && rev);
        uint64_t v = same ? qlen : 0;
        if (m & (m - 1))   // (wave-uniform: the sum over lanes only where a group has more than one)
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == l) {
            lead = true;
            nf = __popcll(m & ~mr);
            nr = __popcll(mr);
            ls = v;
        }
        todo &= ~m;
    }
    if (lead) tally_insert(t, key, nf, nr, ls);
}

// Elements as in k_report.hip: record r's head is element r + melem[r], its markers follow.  E may be an UPPER bound of R + melem[R] (the map's
// scan gives the elements past the end the last record): an element is a marker only below its record's count.
template <bool COMBINE>
__global__ __launch_bounds__(256) void k_tally_add(const TallyTab t, const rbg_report_seed_t *__restrict__ recs, const uint64_t *__restrict__ melem,
                                                   const uint64_t *__restrict__ mk, const uint32_t *__restrict__ erec, const uint64_t R, const uint64_t E) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        atomicAdd(reinterpret_cast<ull *>(t.hdr + 6), static_cast<ull>(R));
        atomicAdd(reinterpret_cast<ull *>(t.hdr + 7), static_cast<ull>(melem[R]));
    }
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
    for (uint64_t e0 = static_cast<uint64_t>(blockIdx.x) * 256; e0 < E; e0 += stride) {   // (every lane of a wave takes the same number of turns)
        const uint64_t e = e0 + threadIdx.x;
        bool active = false, rev = false;
        uint64_t key = 0, qlen = 0;
        if (e < E) {
            const uint64_t r = erec[e], h = r + melem[r], nm = melem[r + 1] - melem[r];
            if (e > h && e - h - 1 < nm) {
                const rbg_report_seed_t x = recs[r];
                key = mk[x.mk_begin + (e - h - 1)];
                rev = x.strand != 0;
                qlen = x.query_len;
                active = true;
            }
        }
        tally_wave_add<COMBINE>(t, active, key, rev, qlen);
    }
}

// ---- per-read mode (rbg_markers_tally_reads, rbg_tally_add_reads_dev) ------------------------------------------------------------------
// The unit of evidence is the read, not the line.  Of all the lines of one read that carry marker m, ONE adds to m's sums: the line with the greatest
// query_len, the earliest in print order among equals.  With SITES, a read whose lines carry two or more alleles of one site (a site is the marker
// without its allele bits, i.e. rotl64(m, 4) >> 4) adds nothing for any marker of that site.
//
// Still one lane per marker element and no sort: an element of record r asks every record r' of its read "do you carry my marker?" by a binary search
// in r's sorted stretch (k_seed_canon leaves every stretch ascending in rotl64(m, 4) and unique), and loses to an r' that does with a greater
// (query_len, -r').  The alleles of one site are neighbours in that order -- the allele is the key's low four bits -- so the site rule is the same
// search for the site's lowest key and a look at up to 16 neighbours; the element's own record is searched like the others.  Cost per element:
// (records of its read) x log2(markers per record) loads.  Every index stays inside [mk_begin, mk_end) whatever the stretch holds: an unsorted
// stretch gives an unspecified table, never an access outside it.

__device__ __forceinline__ uint64_t tally_rotl4(const uint64_t m) { return (m << 4) | (m >> 60); }

// the first index in [b, e) whose key is >= k
__device__ __forceinline__ uint64_t tally_lower(const uint64_t *__restrict__ mk, uint64_t b, uint64_t e, const uint64_t k) {
    while (b < e) {
        const uint64_t mid = b + ((e - b) >> 1);
        if (tally_rotl4(mk[mid]) < k) b = mid + 1; else e = mid;
    }
    return b;
}

// span[r] = the records [a, b) of r's read, from the per-read offsets (rep_off[N + 1], ascending; reads without records are skipped).  Clamped so that
// a <= r < b <= R whatever rep_off holds.
__global__ __launch_bounds__(256) void k_tally_read_spans(const uint64_t *__restrict__ rep_off, const uint64_t N, const uint64_t R, uint2 *__restrict__ span) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; r < R; r += stride) {
        uint64_t lo = 0, hi = N - 1;   // the first read whose records end beyond r
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (rep_off[mid + 1] > r) hi = mid; else lo = mid + 1;
        }
        const uint64_t a = rep_off[lo], b = rep_off[lo + 1];
        span[r] = make_uint2(static_cast<uint32_t>(a < r ? a : r), static_cast<uint32_t>(b <= r ? r + 1 : b < R ? b : R));
    }
}

// xhdr (4 u64): - (the host counts the reads), elements seen, elements that lost to another line of their read, elements dropped by the site rule.
// hdr[7] counts the elements ADDED here (seen = added + lost + dropped).
template <bool COMBINE, bool SITES>
__global__ __launch_bounds__(256) void k_tally_add_reads(const TallyTab t, uint64_t *__restrict__ xhdr, const rbg_report_seed_t *__restrict__ recs,
                                                         const uint64_t *__restrict__ melem, const uint64_t *__restrict__ mk, const uint32_t *__restrict__ erec,
                                                         const uint2 *__restrict__ span, const uint64_t R, const uint64_t E) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        atomicAdd(reinterpret_cast<ull *>(t.hdr + 6), static_cast<ull>(R));
        atomicAdd(reinterpret_cast<ull *>(xhdr + 1), static_cast<ull>(melem[R]));
    }
    uint64_t n_add = 0, n_lost = 0, n_drop = 0;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
    for (uint64_t e0 = static_cast<uint64_t>(blockIdx.x) * 256; e0 < E; e0 += stride) {   // (every lane of a wave takes the same number of turns)
        const uint64_t e = e0 + threadIdx.x;
        bool active = false, rev = false;
        uint64_t key = 0, qlen = 0;
        if (e < E) {
            const uint64_t r = erec[e], h = r + melem[r], nm = melem[r + 1] - melem[r];
            if (e > h && e - h - 1 < nm) {
                const rbg_report_seed_t x = recs[r];
                key = mk[x.mk_begin + (e - h - 1)];
                rev = x.strand != 0;
                qlen = x.query_len;
                const uint64_t k = tally_rotl4(key);
                const uint2 sp = span[r];
                bool lost = false, conflict = false;
                for (uint64_t q = sp.x; q < sp.y; ++q) {
                    if (!SITES && q == r) continue;
                    const uint64_t b = recs[q].mk_begin, end = recs[q].mk_end;
                    if (end <= b) continue;
                    bool has = false;
                    if (SITES) {
                        uint64_t p = tally_lower(mk, b, end, k & ~uint64_t(15));
                        for (int j = 0; j < 16 && p < end; ++j, ++p) {
                            const uint64_t kk = tally_rotl4(mk[p]);
                            if ((kk >> 4) != (k >> 4)) break;
                            if (kk == k) has = true; else conflict = true;
                        }
                        if (conflict) break;
                    } else {
                        const uint64_t p = tally_lower(mk, b, end, k);
                        has = p < end && mk[p] == key;
                    }
                    if (has && q != r) {
                        const uint64_t ql = recs[q].query_len;
                        if (ql > qlen || (ql == qlen && q < r)) {
                            lost = true;
                            if (!SITES) break;
                        }
                    }
                }
                active = !lost && !conflict;
                n_add += active;
                n_drop += conflict;
                n_lost += lost && !conflict;
            }
        }
        tally_wave_add<COMBINE>(t, active, key, rev, qlen);
    }
    for (int o = 32; o > 0; o >>= 1) {
        n_add += __shfl_xor(n_add, o);
        n_lost += __shfl_xor(n_lost, o);
        n_drop += __shfl_xor(n_drop, o);
    }
    if ((threadIdx.x & 63) == 0) {   // one addition per wave and counter
        if (n_add) atomicAdd(reinterpret_cast<ull *>(t.hdr + 7), static_cast<ull>(n_add));
        if (n_lost) atomicAdd(reinterpret_cast<ull *>(xhdr + 2), static_cast<ull>(n_lost));
        if (n_drop) atomicAdd(reinterpret_cast<ull *>(xhdr + 3), static_cast<ull>(n_drop));
    }
}

// (an entry without counts is not part of any export and adds nothing)
__global__ __launch_bounds__(256) void k_tally_add_entries(const TallyTab t, const rbg_tally_entry_t *__restrict__ in, const uint64_t count) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
        const rbg_tally_entry_t x = in[i];
        if (x.n_fwd + x.n_rev) tally_insert(t, x.marker, x.n_fwd, x.n_rev, x.len_sum);
    }
}

__global__ __launch_bounds__(256) void k_tally_rehash(const uint64_t *__restrict__ old_slots, const uint64_t old_cap, const TallyTab t) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < old_cap; i += stride) {
        const uint64_t *s = old_slots + 4 * i;
        if (s[0] != kTallyEmpty) tally_insert(t, s[0], s[1], s[2], s[3]);
    }
}

// an empty table: every key 2^64 - 1, every sum 0 (a claimed slot is only ever added to)
__global__ __launch_bounds__(256) void k_tally_clear(uint64_t *__restrict__ slots, const uint64_t cap) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < 4 * cap; i += stride) slots[i] = (i & 3) ? 0 : kTallyEmpty;
}

__device__ __forceinline__ bool slot_live(const uint64_t *s) { return s[0] != kTallyEmpty && (s[1] + s[2]) != 0; }

__global__ __launch_bounds__(256) void k_tally_live(const uint64_t *__restrict__ slots, const uint64_t cap, uint64_t *__restrict__ pos) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < cap; i += stride) {
        if (i == 0) pos[0] = 0;
        pos[i + 1] = slot_live(slots + 4 * i) ? 1 : 0;
    }
}
// pos: the inclusive sum of k_tally_live behind a leading 0; out has room for pos[cap] + 1 entries (the last one for marker 2^64 - 1)
__global__ __launch_bounds__(256) void k_tally_gather(const TallyTab t, const uint64_t *__restrict__ pos, rbg_tally_entry_t *__restrict__ out) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < t.cap; i += stride) {
        const uint64_t *s = t.slots + 4 * i;
        if (pos[i + 1] != pos[i]) out[pos[i]] = rbg_tally_entry_t{s[0], s[1], s[2], s[3]};
        if (i == 0 && (t.hdr[1] + t.hdr[2]) != 0) out[pos[t.cap]] = rbg_tally_entry_t{kTallyEmpty, t.hdr[1], t.hdr[2], t.hdr[3]};
    }
}

inline int tally_grid(const uint64_t n) { return static_cast<int>(std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), 256ull * 32)); }

}  // namespace

// ---- launchers (all asynchronous on `stream`; hipError_t as int) ---------------------------------------------------------------------

bool tally_combine_default() {
    const char *e = std::getenv("RBG_TALLY_COMBINE");
    return !(e && e[0] == '0');
}

int launch_tally_clear(uint64_t *slots, uint64_t cap, void *stream) {
    hipLaunchKernelGGL(k_tally_clear, dim3(tally_grid(4 * cap)), dim3(256), 0, static_cast<hipStream_t>(stream), slots, cap);
    return static_cast<int>(hipGetLastError());
}

// erec: launch_report_map's element -> record array over E elements (E >= R + melem[R])
int launch_tally_add(uint64_t *slots, uint64_t cap, uint64_t *hdr, const void *recs, const uint64_t *melem, const uint64_t *mk, const uint32_t *erec, uint64_t R,
                     uint64_t E, bool combine, void *stream) {
    const TallyTab t{slots, cap, hdr};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (combine)
        hipLaunchKernelGGL(k_tally_add<true>, dim3(tally_grid(E)), dim3(256), 0, st, t, static_cast<const rbg_report_seed_t *>(recs), melem, mk, erec, R, E);
    else
        hipLaunchKernelGGL(k_tally_add<false>, dim3(tally_grid(E)), dim3(256), 0, st, t, static_cast<const rbg_report_seed_t *>(recs), melem, mk, erec, R, E);
    return static_cast<int>(hipGetLastError());
}

// per-read mode: rep_off[N + 1] the records' per-read offsets (N >= 1), span room for R uint2 (8-byte aligned); flags: RBG_TALLY_PER_READ [| DROP_SITE_CONFLICTS]
int launch_tally_add_reads(uint64_t *slots, uint64_t cap, uint64_t *hdr, uint64_t *xhdr, const void *recs, const uint64_t *melem, const uint64_t *mk,
                           const uint32_t *erec, const uint64_t *rep_off, uint64_t N, void *span, uint64_t R, uint64_t E, uint32_t flags, bool combine, void *stream) {
    const TallyTab t{slots, cap, hdr};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const rbg_report_seed_t *x = static_cast<const rbg_report_seed_t *>(recs);
    uint2 *sp = static_cast<uint2 *>(span);
    hipLaunchKernelGGL(k_tally_read_spans, dim3(tally_grid(R)), dim3(256), 0, st, rep_off, N, R, sp);
    const dim3 grid(tally_grid(E)), block(256);
    const bool sites = (flags & RBG_TALLY_DROP_SITE_CONFLICTS) != 0;
    if (combine && sites) hipLaunchKernelGGL((k_tally_add_reads<true, true>), grid, block, 0, st, t, xhdr, x, melem, mk, erec, sp, R, E);
    else if (combine) hipLaunchKernelGGL((k_tally_add_reads<true, false>), grid, block, 0, st, t, xhdr, x, melem, mk, erec, sp, R, E);
    else if (sites) hipLaunchKernelGGL((k_tally_add_reads<false, true>), grid, block, 0, st, t, xhdr, x, melem, mk, erec, sp, R, E);
    else hipLaunchKernelGGL((k_tally_add_reads<false, false>), grid, block, 0, st, t, xhdr, x, melem, mk, erec, sp, R, E);
    return static_cast<int>(hipGetLastError());
}

int launch_tally_add_entries(uint64_t *slots, uint64_t cap, uint64_t *hdr, const void *entries, uint64_t count, void *stream) {
    if (count == 0) return 0;
    const TallyTab t{slots, cap, hdr};
    hipLaunchKernelGGL(k_tally_add_entries, dim3(tally_grid(count)), dim3(256), 0, static_cast<hipStream_t>(stream), t, static_cast<const rbg_tally_entry_t *>(entries),
                       count);
    return static_cast<int>(hipGetLastError());
}

// new_slots: cleared; the header's claimed count is set anew by the re-insertion (the caller zeroes hdr[5] first)
int launch_tally_rehash(const uint64_t *old_slots, uint64_t old_cap, uint64_t *new_slots, uint64_t new_cap, uint64_t *hdr, void *stream) {
    const TallyTab t{new_slots, new_cap, hdr};
    hipLaunchKernelGGL(k_tally_rehash, dim3(tally_grid(old_cap)), dim3(256), 0, static_cast<hipStream_t>(stream), old_slots, old_cap, t);
    return static_cast<int>(hipGetLastError());
}

size_t tally_compact_tmp_bytes(uint64_t cap) {
    size_t bytes = 0;
    uint64_t *p = nullptr;
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, bytes, p, p, static_cast<int64_t>(cap));
    return bytes + 256;
}
// pos[cap + 1]: pos[i] = live slots before slot i; pos[cap] = their number
// (tmp is the tally's own allocation -- 256-byte aligned, never a caller's pointer: no scan_scratch() needed)
int launch_tally_compact_plan(const uint64_t *slots, uint64_t cap, uint64_t *pos, void *tmp, size_t tmp_bytes, void *stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_tally_live, dim3(tally_grid(cap)), dim3(256), 0, st, slots, cap, pos);
    size_t tb = tmp_bytes;
    const hipError_t e = hipcub::DeviceScan::InclusiveSum(tmp, tb, pos + 1, pos + 1, static_cast<int64_t>(cap), st);
    return static_cast<int>(e != hipSuccess ? e : hipGetLastError());
}
int launch_tally_compact_fill(uint64_t *slots, uint64_t cap, uint64_t *hdr, const uint64_t *pos, void *out, void *stream) {
    const TallyTab t{slots, cap, hdr};
    hipLaunchKernelGGL(k_tally_gather, dim3(tally_grid(cap)), dim3(256), 0, static_cast<hipStream_t>(stream), t, pos, static_cast<rbg_tally_entry_t *>(out));
    return static_cast<int>(hipGetLastError());
}

}  // namespace rbg
