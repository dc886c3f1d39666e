// sa_build.hip -- an index from its text, on the device: the suffix array by prefix doubling over ranks (rbg_suffix_array_dev), then the run-length BWT
// with the suffix-array samples at both ends of every run (rbg_text_runs_plan_dev / rbg_text_runs_fill_dev; include/rbg.h).  Templated on the position
// width only (with_pos): ranks and suffix-array entries take 4 bytes where n < 2^32 - 16, else 8.
//
// The text ends in its unique smallest byte.  k_sa_hist counts the bytes (LDS histogram, one global add per byte value and workgroup) and notes the last
// byte; the host reads the 257 words and refuses a text that breaks the rule before anything is sorted.
//
// A rank is the suffix-array position of the FIRST suffix of its group (Larsson & Sadakane), not a dense number: a group of suffixes that agree on their first
// h symbols occupies positions rank .. rank + size - 1 whatever happens in other groups, so a suffix whose group has one member has its final rank and
// leaves the work list.  Per round, over the m suffixes still listed:
//   round 0   k_sa_key0      key = the first eight bytes, big-endian, zeros behind the text (the terminator is unique: no two keys that reach it agree)
//             sort (key, suffix), k_sa_flags0: head[j] = j where key[j] != key[j - 1], else 0; inclusive max-scan; k_sa_rerank0: rank[suffix] = head, keep =
//             the group has a second member
//   round k   k_sa_keys      key = (rank[i], rank[i + h]) -- one 64-bit word at 4-byte positions; at 8-byte positions two stable sorts, by rank[i + h]
//                            (k_sa_key_lo) and then by rank[i] (k_sa_key_hi).  i + h >= n takes 0: such a suffix reached the terminator and is alone already
//             sort, k_sa_flags: ghead[j] = j where rank[i] changes, shead[j] = j where the pair changes; two max-scans; k_sa_rerank: rank[suffix] =
//             rank[i] + (shead - ghead), keep as above
//   both      inclusive sum of keep, k_sa_compact: the kept suffixes, in order, into the other list; m = the sum's last value (read by the host: one wait per
//             round); h doubles (8 after round 0)
// until the list is empty: the ranks are a permutation and k_sa_scatter writes sa[rank[i]] = i.  Keys are built from the ranks of the round before and
// ranks are written by the re-rank kernel alone, which reads none: a round sees exactly the order by h symbols.  Sorts and scans are hipCUB (DoubleBuffer
// sorts: no hidden copy of the keys); the list of suffixes lives in d_sa and one buffer of the scratch in turn.
//
// Scratch per symbol (sa_layout): rank P + second list P + two key buffers 16 + two scan buffers 2P, P the position width -- 32 bytes at 4-byte
// positions, 48 at 8 -- plus hipCUB's own and 4 KiB of counters.
//
// Runs: k_bwt_flags marks the rows whose BWT byte text[(sa[i] - 1) mod n] differs from the row before (byte 0 reads as 1, as the run builders store it),
// an inclusive sum numbers the runs, k_bwt_fill writes head / first sample at a run's first row and the last sample at its last; the length is the sum of
// -first and last + 1, added by the two rows that know them.
#include <hipcub/hipcub.hpp>

#include "rbg_launch.hpp"

namespace rbg {
namespace {

constexpr uint32_t kSaThreads = 256;
constexpr uint64_t kSaGridCap = 8192;

inline dim3 sa_grid(const uint64_t m) { return dim3(static_cast<uint32_t>(std::max<uint64_t>(1, std::min((m + kSaThreads - 1) / kSaThreads, kSaGridCap)))); }

#define SA_FOR(j, m)                                                                                                        \
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x, stride_ = static_cast<uint64_t>(gridDim.x) * blockDim.x; j < (m); \
         j += stride_)

// hist[0 .. 256) += the count of every byte value (zeroed by the caller); hist[256] = the last byte
__global__ __launch_bounds__(256) void k_sa_hist(const uint8_t *__restrict__ text, const uint64_t n, unsigned long long *__restrict__ hist) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    SA_FOR(i, n) atomicAdd(&h[text[i]], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], static_cast<unsigned long long>(h[threadIdx.x]));
    if (blockIdx.x == 0 && threadIdx.x == 0) hist[256] = text[n - 1];
}

template <typename P>
__global__ __launch_bounds__(256) void k_sa_key0(const uint8_t *__restrict__ text, const uint64_t n, uint64_t *__restrict__ keys, P *__restrict__ idx) {
    SA_FOR(i, n) {
        uint64_t k = 0;
#pragma unroll
        for (uint32_t d = 0; d < 8; ++d) k = (k << 8) | (i + d < n ? static_cast<uint64_t>(text[i + d]) : 0ull);
        keys[i] = k;
        idx[i] = static_cast<P>(i);
    }
}

template <typename P>
__global__ __launch_bounds__(256) void k_sa_flags0(const uint64_t *__restrict__ keys, const uint64_t m, P *__restrict__ head) {
    SA_FOR(j, m) head[j] = (j == 0 || keys[j] != keys[j - 1]) ? static_cast<P>(j) : P(0);
}

// head: scanned.  keep[j] = 1 while the group of j has a second member
template <typename P>
__global__ __launch_bounds__(256) void k_sa_rerank0(const P *__restrict__ head, const P *__restrict__ idx, const uint64_t m, P *__restrict__ rank,
                                                    P *__restrict__ keep) {
    SA_FOR(j, m) {
        const P h = head[j];
        rank[idx[j]] = h;
        const bool single = h == j && (j + 1 == m || head[j + 1] == j + 1);
        keep[j] = single ? P(0) : P(1);
    }
}

// the pair a listed suffix is sorted by: its rank and the rank h symbols further on
template <typename P>
__device__ __forceinline__ void sa_pair(const P *__restrict__ rank, const uint64_t i, const uint64_t n, const uint64_t h, uint64_t &r1, uint64_t &r2) {
    r1 = rank[i];
    r2 = h < n - i ? static_cast<uint64_t>(rank[i + h]) : 0ull;      // (i < n; written so that a large h does not wrap)
}

__global__ __launch_bounds__(256) void k_sa_keys(const uint32_t *__restrict__ rank, const uint32_t *__restrict__ act, const uint64_t m, const uint64_t n,
                                                 const uint64_t h, uint64_t *__restrict__ keys) {
    SA_FOR(j, m) {
        uint64_t r1, r2;
        sa_pair<uint32_t>(rank, act[j], n, h, r1, r2);
        keys[j] = (r1 << 32) | r2;
    }
}

__global__ __launch_bounds__(256) void k_sa_key_lo(const uint64_t *__restrict__ rank, const uint64_t *__restrict__ act, const uint64_t m, const uint64_t n,
                                                   const uint64_t h, uint64_t *__restrict__ keys) {
    SA_FOR(j, m) {
        uint64_t r1, r2;
        sa_pair<uint64_t>(rank, act[j], n, h, r1, r2);
        keys[j] = r2;
    }
}

__global__ __launch_bounds__(256) void k_sa_key_hi(const uint64_t *__restrict__ rank, const uint64_t *__restrict__ act, const uint64_t m,
                                                   uint64_t *__restrict__ keys) {
    SA_FOR(j, m) keys[j] = rank[act[j]];
}

// the sorted pair at j: at 4-byte positions the key itself; at 8-byte positions the key is rank[i] and rank[i + h] is read again
template <typename P>
__device__ __forceinline__ void sa_sorted_pair(const uint64_t *__restrict__ keys, const P *__restrict__ idx, const P *__restrict__ rank, const uint64_t n,
                                               const uint64_t h, const uint64_t j, uint64_t &r1, uint64_t &r2) {
    if constexpr (sizeof(P) == 4) {
        r1 = keys[j] >> 32;
        r2 = keys[j] & 0xFFFFFFFFull;
    } else {
        const uint64_t i = idx[j];
        r1 = keys[j];
        r2 = h < n - i ? rank[i + h] : 0ull;
    }
}

template <typename P>
__global__ __launch_bounds__(256) void k_sa_flags(const uint64_t *__restrict__ keys, const P *__restrict__ idx, const P *__restrict__ rank, const uint64_t m,
                                                  const uint64_t n, const uint64_t h, P *__restrict__ ghead, P *__restrict__ shead) {
    SA_FOR(j, m) {
        P g = 0, s = 0;
        if (j) {
            uint64_t a1, a2, b1, b2;
            sa_sorted_pair<P>(keys, idx, rank, n, h, j, a1, a2);
            sa_sorted_pair<P>(keys, idx, rank, n, h, j - 1, b1, b2);
            if (a1 != b1) g = static_cast<P>(j);
            if (a1 != b1 || a2 != b2) s = static_cast<P>(j);
        }
        ghead[j] = g;
        shead[j] = s;
    }
}

// ghead, shead: scanned.  The new rank goes to rank[]; ghead[j] becomes keep[j] (each lane reads its own ghead[j] only)
template <typename P>
__global__ __launch_bounds__(256) void k_sa_rerank(const uint64_t *__restrict__ keys, const P *__restrict__ idx, P *__restrict__ ghead,
                                                   const P *__restrict__ shead, const uint64_t m, P *__restrict__ rank) {
    SA_FOR(j, m) {
        const uint64_t r1 = sizeof(P) == 4 ? keys[j] >> 32 : keys[j];
        const P s = shead[j], g = ghead[j];
        rank[idx[j]] = static_cast<P>(r1 + (s - g));
        const bool single = s == j && (j + 1 == m || shead[j + 1] == j + 1);
        ghead[j] = single ? P(0) : P(1);
    }
}

// incl = the inclusive sum of keep: the kept suffixes, in order, into out[0 .. incl[m - 1])
template <typename P>
__global__ __launch_bounds__(256) void k_sa_compact(const P *__restrict__ incl, const P *__restrict__ idx, const uint64_t m, P *__restrict__ out) {
    SA_FOR(j, m) {
        const P c = incl[j], before = j ? incl[j - 1] : P(0);
        if (c != before) out[c - 1] = idx[j];
    }
}

template <typename P>
__global__ __launch_bounds__(256) void k_sa_scatter(const P *__restrict__ rank, const uint64_t n, P *__restrict__ sa) {
    SA_FOR(i, n) sa[rank[i]] = static_cast<P>(i);
}

template <typename P>
__device__ __forceinline__ uint32_t bwt_at(const uint8_t *__restrict__ text, const P *__restrict__ sa, const uint64_t n, const uint64_t i) {
    const uint64_t p = sa[i];
    const uint32_t c = text[p && p < n ? p - 1 : n - 1];      // (a value that is no text position reads as 0: never out of bounds)
    return c ? c : 1u;
}

template <typename P>
__global__ __launch_bounds__(256) void k_bwt_flags(const uint8_t *__restrict__ text, const P *__restrict__ sa, const uint64_t n, P *__restrict__ flag) {
    SA_FOR(i, n) flag[i] = (i == 0 || bwt_at<P>(text, sa, n, i) != bwt_at<P>(text, sa, n, i - 1)) ? P(1) : P(0);
}

// run = the inclusive sum of the flags; lens zeroed by the caller
template <typename P>
__global__ __launch_bounds__(256) void k_bwt_fill(const uint8_t *__restrict__ text, const P *__restrict__ sa, const uint64_t n, const P *__restrict__ run,
                                                  const uint64_t R, uint8_t *__restrict__ heads, unsigned long long *__restrict__ lens,
                                                  uint64_t *__restrict__ ssa, uint64_t *__restrict__ esa) {
    SA_FOR(i, n) {
        const uint64_t id = static_cast<uint64_t>(run[i]) - 1;
        if (id >= R) continue;      // (a run count that is not the plan's: nothing is written out of bounds)
        if (i == 0 || run[i - 1] != run[i]) {
            heads[id] = static_cast<uint8_t>(bwt_at<P>(text, sa, n, i));
            ssa[id] = sa[i];
            atomicAdd(&lens[id], 0ull - i);
        }
        if (i + 1 == n || run[i + 1] != run[i]) {
            esa[id] = sa[i];
            atomicAdd(&lens[id], i + 1);
        }
    }
}

inline size_t up256(const size_t b) { return (b + 255) & ~size_t(255); }

struct SaLayout {
    size_t rank, idx, key_a, key_b, scan_a, scan_b, small, cub, cub_bytes, total;
};

template <typename P>
size_t sa_cub_bytes(const uint64_t n) {
    const int64_t m = static_cast<int64_t>(n ? n : 1);
    size_t a = 0, b = 0, c = 0;
    hipcub::DoubleBuffer<uint64_t> dk(nullptr, nullptr);
    hipcub::DoubleBuffer<P> dv(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, dk, dv, m, 0, 64);
    (void)hipcub::DeviceScan::InclusiveScan(nullptr, b, static_cast<P *>(nullptr), static_cast<P *>(nullptr), hipcub::Max(), m);
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, c, static_cast<P *>(nullptr), static_cast<P *>(nullptr), m);
    return std::max(a, std::max(b, c));
}

SaLayout sa_layout(const uint64_t n, const uint32_t pos_bytes) {
    SaLayout L{};
    const size_t np = up256(static_cast<size_t>(n) * pos_bytes), nk = up256(static_cast<size_t>(n) * 8);
    size_t at = 0;
    L.rank = at, at += np;
    L.idx = at, at += np;
    L.key_a = at, at += nk;
    L.key_b = at, at += nk;
    L.scan_a = at, at += np;
    L.scan_b = at, at += np;
    L.small = at, at += 4096;
    L.cub = at;
    L.cub_bytes = up256(with_pos(pos_bytes, [&](auto p) { return sa_cub_bytes<pos_t<decltype(p)>>(n); }));
    L.total = at + L.cub_bytes;
    return L;
}

struct RunsLayout {
    size_t scan, cub, cub_bytes, total;
};

RunsLayout runs_layout(const uint64_t n, const uint32_t pos_bytes) {
    RunsLayout L{};
    L.scan = 0;
    L.cub = up256(static_cast<size_t>(n) * pos_bytes);
    L.cub_bytes = up256(with_pos(pos_bytes, [&](auto p) {
        using P = pos_t<decltype(p)>;
        size_t b = 0;
        (void)hipcub::DeviceScan::InclusiveSum(nullptr, b, static_cast<P *>(nullptr), static_cast<P *>(nullptr), static_cast<int64_t>(n ? n : 1));
        return b;
    }));
    L.total = L.cub + L.cub_bytes;
    return L;
}

inline uint32_t bit_length(uint64_t v) {
    uint32_t b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

#define SA_HIP(expr)                                   \
    do {                                               \
        if ((expr) != hipSuccess) {                    \
            (void)hipGetLastError();                   \
            return 2;                                  \
        }                                              \
    } while (0)
#define SA_LAUNCH(expr)                                \
    do {                                               \
        if (expr) return 2;                            \
    } while (0)

template <typename P>
int sa_build_t(const uint8_t *text, const uint64_t n, P *sa, uint8_t *tmp, const SaLayout &L, hipStream_t st, uint64_t info[8]) {
    const dim3 block(kSaThreads);
    unsigned long long *hist = reinterpret_cast<unsigned long long *>(tmp + L.small);
    SA_HIP(hipMemsetAsync(hist, 0, 257 * 8, st));
    SA_LAUNCH(launch_grid(k_sa_hist, sa_grid(n), block, 0, st, text, n, hist));
    unsigned long long hh[257];
    SA_HIP(hipMemcpyAsync(hh, hist, sizeof hh, hipMemcpyDeviceToHost, st));
    SA_HIP(hipStreamSynchronize(st));
    uint32_t least = 0;
    while (least < 256 && hh[least] == 0) ++least;
    if (least == 256 || hh[least] != 1 || hh[256] != least) return 1;      // the last byte is not the unique smallest: nothing is sorted

    P *rank = reinterpret_cast<P *>(tmp + L.rank);
    P *scan_a = reinterpret_cast<P *>(tmp + L.scan_a), *scan_b = reinterpret_cast<P *>(tmp + L.scan_b);
    hipcub::DoubleBuffer<uint64_t> keys(reinterpret_cast<uint64_t *>(tmp + L.key_a), reinterpret_cast<uint64_t *>(tmp + L.key_b));
    hipcub::DoubleBuffer<P> list(sa, reinterpret_cast<P *>(tmp + L.idx));
    void *cub = tmp + L.cub;
    size_t cb = L.cub_bytes;
    const int pos_bits = static_cast<int>(bit_length(n - 1));
    uint64_t m = n, rounds = 0, sorted = 0, h = 8;

    // the end of every round: keep -> its inclusive sum, the kept suffixes into the other list, their number to the host
    auto shrink = [&](P *keep) -> int {
        cb = L.cub_bytes;
        SA_HIP(hipcub::DeviceScan::InclusiveSum(cub, cb, keep, keep, static_cast<int64_t>(m), st));
        SA_LAUNCH(launch_grid(k_sa_compact<P>, sa_grid(m), block, 0, st, static_cast<const P *>(keep), static_cast<const P *>(list.Current()), m,
                              list.Alternate()));
        P kept = 0;
        SA_HIP(hipMemcpyAsync(&kept, keep + (m - 1), sizeof(P), hipMemcpyDeviceToHost, st));
        SA_HIP(hipStreamSynchronize(st));
        list.selector ^= 1;
        m = kept;
        return 0;
    };

    SA_LAUNCH(launch_grid(k_sa_key0<P>, sa_grid(n), block, 0, st, text, n, keys.Current(), list.Current()));
    cb = L.cub_bytes;
    SA_HIP(hipcub::DeviceRadixSort::SortPairs(cub, cb, keys, list, static_cast<int64_t>(n), 0, 64, st));
    SA_LAUNCH(launch_grid(k_sa_flags0<P>, sa_grid(n), block, 0, st, static_cast<const uint64_t *>(keys.Current()), n, scan_a));
    cb = L.cub_bytes;
    SA_HIP(hipcub::DeviceScan::InclusiveScan(cub, cb, scan_a, scan_a, hipcub::Max(), static_cast<int64_t>(n), st));
    SA_LAUNCH(launch_grid(k_sa_rerank0<P>, sa_grid(n), block, 0, st, static_cast<const P *>(scan_a), static_cast<const P *>(list.Current()), n, rank, scan_b));
    rounds = 1;
    sorted = n;
    if (int rc = shrink(scan_b)) return rc;
    info[5] = m;

    while (m) {
        if (rounds > 70) return 2;      // (h has passed 2^64: the ranks cannot still be tied)
        const P *crank = rank;
        if constexpr (sizeof(P) == 4) {
            SA_LAUNCH(launch_grid(k_sa_keys, sa_grid(m), block, 0, st, crank, static_cast<const P *>(list.Current()), m, n, h, keys.Current()));
            cb = L.cub_bytes;
            SA_HIP(hipcub::DeviceRadixSort::SortPairs(cub, cb, keys, list, static_cast<int64_t>(m), 0, 32 + pos_bits, st));
        } else {
            SA_LAUNCH(launch_grid(k_sa_key_lo, sa_grid(m), block, 0, st, crank, static_cast<const P *>(list.Current()), m, n, h, keys.Current()));
            cb = L.cub_bytes;
            SA_HIP(hipcub::DeviceRadixSort::SortPairs(cub, cb, keys, list, static_cast<int64_t>(m), 0, std::max(pos_bits, 1), st));
            SA_LAUNCH(launch_grid(k_sa_key_hi, sa_grid(m), block, 0, st, crank, static_cast<const P *>(list.Current()), m, keys.Current()));
            cb = L.cub_bytes;
            SA_HIP(hipcub::DeviceRadixSort::SortPairs(cub, cb, keys, list, static_cast<int64_t>(m), 0, std::max(pos_bits, 1), st));
        }
        SA_LAUNCH(launch_grid(k_sa_flags<P>, sa_grid(m), block, 0, st, static_cast<const uint64_t *>(keys.Current()), static_cast<const P *>(list.Current()), crank,
                              m, n, h, scan_b, scan_a));
        cb = L.cub_bytes;
        SA_HIP(hipcub::DeviceScan::InclusiveScan(cub, cb, scan_a, scan_a, hipcub::Max(), static_cast<int64_t>(m), st));
        cb = L.cub_bytes;
        SA_HIP(hipcub::DeviceScan::InclusiveScan(cub, cb, scan_b, scan_b, hipcub::Max(), static_cast<int64_t>(m), st));
        SA_LAUNCH(launch_grid(k_sa_rerank<P>, sa_grid(m), block, 0, st, static_cast<const uint64_t *>(keys.Current()), static_cast<const P *>(list.Current()),
                              scan_b, static_cast<const P *>(scan_a), m, rank));
        rounds += 1;
        sorted += m;
        if (int rc = shrink(scan_b)) return rc;
        h = h > (~0ull >> 1) ? ~0ull : h * 2;
    }
    SA_LAUNCH(launch_grid(k_sa_scatter<P>, sa_grid(n), block, 0, st, static_cast<const P *>(rank), n, sa));
    info[0] = rounds;
    info[1] = sorted;
    return 0;
}

}  // namespace

size_t sa_tmp_bytes(uint64_t n, uint32_t pos_bytes) { return sa_layout(n, pos_bytes).total; }

// 0: done; 1: the text's last byte is not its unique smallest (nothing written to sa); 2: a HIP error.  info: rounds, elements sorted per round summed, scratch
// bytes, n, pos_bytes, suffixes still listed after round 0.  Waits for the stream once per round.
int sa_build(const uint8_t *text, uint64_t n, void *sa, uint32_t pos_bytes, void *tmp, size_t tmp_bytes, void *stream, uint64_t info[8]) {
    const SaLayout L = sa_layout(n, pos_bytes);
    if (n == 0 || tmp_bytes < L.total) return 2;
    for (int k = 0; k < 8; ++k) info[k] = 0;
    info[2] = L.total;
    info[3] = n;
    info[4] = pos_bytes;
    return with_pos(pos_bytes, [&](auto p) {
        using P = pos_t<decltype(p)>;
        return sa_build_t<P>(text, n, static_cast<P *>(sa), static_cast<uint8_t *>(tmp), L, static_cast<hipStream_t>(stream), info);
    });
}

size_t text_runs_tmp_bytes(uint64_t n, uint32_t pos_bytes) { return runs_layout(n, pos_bytes).total; }

// the runs of the BWT numbered in tmp; *R = their count (waits for the stream).  0 or 2 as sa_build
int text_runs_plan(const uint8_t *text, const void *sa, uint64_t n, uint32_t pos_bytes, void *tmp, size_t tmp_bytes, uint64_t *R, void *stream) {
    const RunsLayout L = runs_layout(n, pos_bytes);
    if (n == 0 || tmp_bytes < L.total) return 2;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_pos(pos_bytes, [&](auto p) -> int {
        using P = pos_t<decltype(p)>;
        P *run = reinterpret_cast<P *>(static_cast<uint8_t *>(tmp) + L.scan);
        SA_LAUNCH(launch_grid(k_bwt_flags<P>, sa_grid(n), dim3(kSaThreads), 0, st, text, static_cast<const P *>(sa), n, run));
        size_t cb = L.cub_bytes;
        SA_HIP(hipcub::DeviceScan::InclusiveSum(static_cast<uint8_t *>(tmp) + L.cub, cb, run, run, static_cast<int64_t>(n), st));
        P last = 0;
        SA_HIP(hipMemcpyAsync(&last, run + (n - 1), sizeof(P), hipMemcpyDeviceToHost, st));
        SA_HIP(hipStreamSynchronize(st));
        *R = last;
        return 0;
    });
}

int text_runs_fill(const uint8_t *text, const void *sa, uint64_t n, uint32_t pos_bytes, const void *tmp, size_t tmp_bytes, uint64_t R, uint8_t *heads,
                   uint64_t *lens, uint64_t *ssa, uint64_t *esa, void *stream) {
    const RunsLayout L = runs_layout(n, pos_bytes);
    if (n == 0 || R == 0 || R > n || tmp_bytes < L.total) return 2;
    hipStream_t st = static_cast<hipStream_t>(stream);
    SA_HIP(hipMemsetAsync(lens, 0, R * 8, st));
    return with_pos(pos_bytes, [&](auto p) -> int {
        using P = pos_t<decltype(p)>;
        const P *run = reinterpret_cast<const P *>(static_cast<const uint8_t *>(tmp) + L.scan);
        SA_LAUNCH(launch_grid(k_bwt_fill<P>, sa_grid(n), dim3(kSaThreads), 0, st, text, static_cast<const P *>(sa), n, run, R, heads,
                              reinterpret_cast<unsigned long long *>(lens), ssa, esa));
        return 0;
    });
}

}  // namespace rbg
