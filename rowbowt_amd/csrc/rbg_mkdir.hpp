// rbg_mkdir.hpp -- the marker directory: its bucket shift, the bucket entries and the 32-byte bucket records (MkRec) as upload_marker_table
// (capi/upload_runs.ipp) builds them, the gates that decide whether records are built, and the arithmetic with which marker_query
// (rbg_device.hpp) answers from two records or from the directory and the run arrays.  Host and device share this text; a host compiler
// takes it alone (tests/cpp/mkrec_check.cpp drives builder and answer against a scan over the runs).
#ifndef RBG_MKDIR_HPP
#define RBG_MKDIR_HPP
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RBG_MK_D __device__ __forceinline__
#else
#define RBG_MK_D inline
#endif

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rbg {

// One 32-byte record per bucket of the marker directory (round 6): at_range(lo, hi) -- MarkerArray::at_range as rowbowt.hpp:272-290 / :437-441 call it -- from the
// records of the buckets of lo and hi, ONE or two sectors, instead of a directory entry, the run ends, the run starts and the value offsets (4.9 sectors per query,
// a third of the marker seeds' misses: profiles/r06_pmc_markers.txt).  `a` = the first run whose end is >= the bucket's first row (what mk_bucket holds), its value
// offset, and EVERY run from `a` on that starts before the bucket's end, as {start, end} relative to the bucket's first row (start clamped to 0 from below, end to
// 0xFFFF from above) and its number of values.  Runs are disjoint and ascending, so for lo in this bucket the first run with end >= lo is a + #{listed: end < lo},
// and for hi in this bucket one past the last run with start <= hi is a + #{listed: start <= hi}; the value offsets follow from off_a and the listed counts.
// nin == kMkRecOverflow: more than kMkRecRuns such runs, or a run with more than 65535 values: the arrays answer (from `a`, as before).
constexpr uint32_t kMkRecRuns = 3, kMkRecOverflow = 0xFF;
struct MkRec {
    uint32_t a;
    uint32_t off_lo;
    uint8_t off_hi, nin;
    uint16_t s_off[kMkRecRuns], e_off[kMkRecRuns], cnt[kMkRecRuns];
    uint16_t pad[2];
};
static_assert(sizeof(MkRec) == 32, "two marker records per 64-byte sector");

// one marker table as the query sees it: the SA-row table (DevIndex::mk_*) or the text-position table (DevIndex::tmk_*), and the length of its key space
struct MkView {
    const uint64_t *start, *end, *off, *vals;
    uint64_t nruns, n;
    const uint32_t *bucket;
    const MkRec *rec;
    uint32_t shift;
};

// ---- the host side: shift, directory, records, gates ----------------------------------------------------------------------------------
// about two buckets per run: at_range's two predecessor searches (2 x log2(nruns) dependent
// loads) become one table read and a scan over the runs of one bucket
inline uint32_t mk_dir_shift(uint64_t n, uint64_t nruns) {
    uint32_t shift = 0;
    while (shift < 20 && (n >> shift) > 2 * nruns) ++shift;
    return shift;
}
inline uint64_t mk_dir_buckets(uint64_t n, uint32_t shift) { return (n >> shift) + 2; }
// bucket[b] = the first run whose end is >= b << shift (nruns if none)
inline void mk_build_dir(const uint64_t *end, uint64_t nruns, uint64_t n, uint32_t shift, std::vector<uint32_t> &bucket) {
    const uint64_t nb = mk_dir_buckets(n, shift);
    bucket.resize(nb);
    uint64_t j = 0;
    for (uint64_t b = 0; b < nb; ++b) {
        const uint64_t first_row = b << shift;
        while (j < nruns && end[j] < first_row) ++j;
        bucket[b] = static_cast<uint32_t>(j);
    }
}
// the bucket records (32 bytes per bucket = about 64 per marker run) are built only while that is a small part of the device -- at most an eighth of the free HBM
// and 16 GB; a marker array of 1e9 runs keeps the 4-byte directory -- for buckets of at most 2^16 rows (s_off, e_off), value offsets below 2^40 (off_hi), and
// unless RBG_MK_REC=0 asks for the arrays only (A/B, tests)
inline bool mk_rec_shift_ok(uint32_t shift) { return shift <= 16; }
inline bool mk_rec_vals_ok(uint64_t nvals) { return (nvals >> 40) == 0; }
inline bool mk_rec_switch_on(const char *env) { return !(env && env[0] == '0'); }
inline bool mk_rec_fits(uint64_t nb, size_t free_bytes) { return nb * sizeof(MkRec) <= std::min<size_t>(free_bytes / 8, size_t(16) << 30); }
inline bool mk_rec_wanted(uint32_t shift, const char *env, uint64_t nvals, uint64_t nb, size_t free_bytes) {
    return mk_rec_shift_ok(shift) && mk_rec_switch_on(env) && mk_rec_vals_ok(nvals) && mk_rec_fits(nb, free_bytes);
}
// off has nruns + 1 entries; nvals = the number of values
inline void mk_build_recs(const uint64_t *start, const uint64_t *end, const uint64_t *off, uint64_t nruns, uint64_t nvals, uint32_t shift,
                          const std::vector<uint32_t> &bucket, std::vector<MkRec> &recs) {
    const uint64_t nb = bucket.size();
    recs.resize(nb);
    for (uint64_t b = 0; b < nb; ++b) {
        MkRec &R = recs[b];
        std::memset(&R, 0, sizeof(R));
        const uint64_t a = bucket[b], first_row = b << shift, end_row = first_row + (uint64_t(1) << shift);
        R.a = static_cast<uint32_t>(a);
        const uint64_t off_a = a < nruns ? off[a] : nvals;
        R.off_lo = static_cast<uint32_t>(off_a);
        R.off_hi = static_cast<uint8_t>(off_a >> 32);
        uint32_t k = 0;
        bool over = false;
        for (uint64_t j2 = a; j2 < nruns && start[j2] < end_row; ++j2) {
            const uint64_t c = off[j2 + 1] - off[j2];
            if (k == kMkRecRuns || c > 0xFFFF) { over = true; break; }
            R.s_off[k] = static_cast<uint16_t>(start[j2] > first_row ? start[j2] - first_row : 0);
            R.e_off[k] = static_cast<uint16_t>(std::min<uint64_t>(end[j2] - first_row, 0xFFFF));   // (end >= first_row: j2 >= a)
            R.cnt[k] = static_cast<uint16_t>(c);
            ++k;
        }
        R.nin = over ? static_cast<uint8_t>(kMkRecOverflow) : static_cast<uint8_t>(k);
    }
}

// ---- the query side --------------------------------------------------------------------------------------------------------------------
// st slot of the run starts / ends read (kStatSearchN + 2; rbg_dev.h asserts it)
constexpr uint32_t kMkStatRuns = 10;
// from the records R0 of lo's bucket and R1 of hi's, neither of them an overflowing one (nin == kMkRecOverflow: the arrays answer, marker_query decides), and
// lo_rel / hi_rel = lo / hi relative to their bucket's first row: f = the first run with end >= lo, l = one past the last run with start <= hi, and the value
// offsets off_f, off_l of both, which it declares.  As text, because marker_query expands it in place: behind a call, even a force-inlined one, hipcc allots the
// registers of seven marker kernels differently (up to nine more SGPRs, one more VGPR in k_find_range_markers); mk_rec_answer is the same text as a function.
#if defined(__HIPCC__)
#define RBG_MK_UNROLL _Pragma("unroll")
#else
#define RBG_MK_UNROLL
#endif
#define RBG_MK_REC_ANSWER(R0, R1, lo_rel, hi_rel, f, l, off_f, off_l)                                                             \
    uint64_t off_f = static_cast<uint64_t>((R0).off_lo) | (static_cast<uint64_t>((R0).off_hi) << 32);                             \
    uint64_t off_l = static_cast<uint64_t>((R1).off_lo) | (static_cast<uint64_t>((R1).off_hi) << 32);                             \
    uint32_t nf = 0, nl = 0;                                                                                                      \
    RBG_MK_UNROLL                                                                                                                 \
    for (uint32_t j = 0; j < kMkRecRuns; ++j) {                                                                                   \
        const bool bf = j < (R0).nin && (R0).e_off[j] < (lo_rel);      /* (ends ascend: a prefix of the listed runs) */           \
        const bool bl = j < (R1).nin && (R1).s_off[j] <= (hi_rel);     /* (starts ascend) */                                      \
        nf += bf ? 1u : 0u; off_f += bf ? (R0).cnt[j] : 0u;                                                                       \
        nl += bl ? 1u : 0u; off_l += bl ? (R1).cnt[j] : 0u;                                                                       \
    }                                                                                                                             \
    f = static_cast<uint64_t>((R0).a) + nf;                                                                                       \
    l = static_cast<uint64_t>((R1).a) + nl;
inline void mk_rec_answer(const MkRec &R0, const MkRec &R1, uint32_t lo_rel, uint32_t hi_rel, uint64_t *first, uint64_t *last, uint64_t *off_first, uint64_t *off_last) {
    RBG_MK_REC_ANSWER(R0, R1, lo_rel, hi_rel, *first, *last, off_f, off_l)
    *off_first = off_f;
    *off_last = off_l;
}
// from the run arrays: a = a run at or before the first one with end >= lo, z = a run at or before one past the last one with start <= hi
RBG_MK_D void marker_span_arrays(const MkView &v, uint64_t lo, uint64_t hi, uint64_t a, uint64_t z, uint64_t *first, uint64_t *last, unsigned long long *st) {
    while (a < v.nruns && v.end[a] < lo) { ++a; if (st) st[kMkStatRuns] += 1; }
    *first = a;
    if (z < a) z = a;
    while (z < v.nruns && v.start[z] <= hi) { ++z; if (st) st[kMkStatRuns] += 1; }
    *last = z;
    if (st) st[kMkStatRuns] += 2;
}

}  // namespace rbg
#endif
