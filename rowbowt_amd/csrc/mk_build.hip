// mk_build.hip -- the marker array of an index from the variant sites of its text, on the device, while the suffix array is still there
// (rbg_marker_runs_plan_dev / rbg_marker_runs_fill_dev; include/rbg.h).  Templated on the position width only (with_pos), like sa_build.hip.
//
// A site record is (pos, first, val): the row i with p = sa[i] carries the values of the records with first <= p <= pos.  pos is strictly ascending and
// first does not descend, so those records are the stretch [lower bound of p in pos, upper bound of p in first) of the list, at most w long.  No inverse
// suffix array is made: the records mark the text positions they cover in a bitmap of n bits, and one coalesced sweep over sa tests a bit per row.
//   k_mk_cover     one lane per record: the rule about the records is checked (hdr.err) and the bits [first, pos] are set (one or two 64-bit atomic ORs)
//   k_mk_count     per chunk of 256 rows (one workgroup trip): the covered rows, counted; then one exclusive sum over the chunks
//   k_mk_compact   the same sweep again: a covered row takes its place in row order (chunk offset + its rank in the workgroup), finds its stretch and
//                  stores {row, first record | count << 56}
// and everything after that works on the C covered rows only (C <= S * w):
//   k_mk_heads     head[j] = the row starts a run: not (adjacent to the covered row before it, both with one value, the same value)
//                  two inclusive sums: the run number, and the values of the run heads
//   k_mk_fill      a run's first row writes run_start, mk_off and its values, sorted by a compare-exchange network over registers (W = 4, 16 or 64 slots,
//                  the smallest that holds w; empty slots hold the largest value and stay behind); its last row writes run_end
// The plan ends by sealing a header in the scratch -- {magic, n, S, w and width, C, nruns, nvals} -- that the fill reads back before it launches anything:
// counts that are not the plan's, or a scratch no plan filled, are refused on the host.
//
// Scratch (mk_layout): 256 bytes of header, n / 8 bytes of bitmap, 8 bytes per chunk of 256 rows, 32 bytes per row that can be covered (min(n, S * w)),
// hipCUB's own.  Every kernel strides a grid capped at kMkGridCap workgroups.
#include <hipcub/hipcub.hpp>

#include "rbg_launch.hpp"

namespace rbg {
namespace {

constexpr uint32_t kMkThreads = 256;
constexpr uint64_t kMkGridCap = 2048;      // tests/test_gpu_marker_build.py: CAP = 2048 * 256 rows per grid pass
constexpr uint64_t kMkMagic = 0x31764B4D52474252ull;
constexpr uint64_t kMkLoMask = (1ull << 56) - 1;

struct MkHeader {
    uint64_t magic, n, S, w_pb, C, nruns, nvals, err;
};

inline dim3 mk_grid(const uint64_t m) { return dim3(static_cast<uint32_t>(std::max<uint64_t>(1, std::min((m + kMkThreads - 1) / kMkThreads, kMkGridCap)))); }

#define MK_FOR(j, m)                                                                                                        \
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x, stride_ = static_cast<uint64_t>(gridDim.x) * blockDim.x; j < (m); \
         j += stride_)

__global__ __launch_bounds__(256) void k_mk_cover(const uint64_t *__restrict__ pos, const uint64_t *__restrict__ first, const uint64_t S, const uint64_t n,
                                                  const uint32_t w, unsigned long long *__restrict__ bits, unsigned long long *__restrict__ err) {
    MK_FOR(r, S) {
        const uint64_t p = pos[r], f = first[r];
        bool bad = p >= n || f > p || p - f >= w;
        if (r && (pos[r - 1] >= p || first[r - 1] > f)) bad = true;
        if (bad) {      // (nothing is set for it: a record that breaks the rule never reaches past the bitmap)
            atomicOr(err, 1ull);
            continue;
        }
        const uint64_t a = f >> 6, b = p >> 6;
        const unsigned long long from = ~0ull << (f & 63), upto = ~0ull >> (63 - (p & 63));
        if (a == b) {
            atomicOr(&bits[a], from & upto);
        } else {      // (w <= 64: two words at the most)
            atomicOr(&bits[a], from);
            atomicOr(&bits[b], upto);
        }
    }
}

template <typename P>
__device__ __forceinline__ bool mk_covered(const P *__restrict__ sa, const unsigned long long *__restrict__ bits, const uint64_t n, const uint64_t i, uint64_t &p) {
    if (i >= n) return false;
    p = sa[i];
    return p < n && ((bits[p >> 6] >> (p & 63)) & 1ull);      // (a value that is no text position is not covered: never out of bounds)
}

// counts[c] = the covered rows of chunk c = rows [256 c, 256 c + 256)
template <typename P>
__global__ __launch_bounds__(256) void k_mk_count(const P *__restrict__ sa, const unsigned long long *__restrict__ bits, const uint64_t n, const uint64_t nchunks,
                                                  uint64_t *__restrict__ counts) {
    for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        uint64_t p;
        const int k = __syncthreads_count(mk_covered<P>(sa, bits, n, c * kMkThreads + threadIdx.x, p));
        if (threadIdx.x == 0) counts[c] = static_cast<uint64_t>(k);
    }
}

// offs: the exclusive sum of counts.  The covered rows in row order, each with its stretch of the record list
template <typename P>
__global__ __launch_bounds__(256) void k_mk_compact(const P *__restrict__ sa, const unsigned long long *__restrict__ bits, const uint64_t n,
                                                    const uint64_t nchunks, const uint64_t *__restrict__ offs, const uint64_t *__restrict__ pos,
                                                    const uint64_t *__restrict__ first, const uint64_t S, const uint32_t w, const uint64_t cap,
                                                    uint64_t *__restrict__ crow, uint64_t *__restrict__ clo) {
    __shared__ uint32_t wave_count[kMkThreads / 64];
    const uint32_t wave = threadIdx.x >> 6;
    for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const uint64_t i = c * kMkThreads + threadIdx.x;
        uint64_t p = 0;
        const bool cov = mk_covered<P>(sa, bits, n, i, p);
        const unsigned long long vote = __ballot(cov);
        const uint32_t before = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(vote >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(vote), 0u));
        if ((threadIdx.x & 63) == 0) wave_count[wave] = static_cast<uint32_t>(__popcll(vote));
        __syncthreads();
        uint64_t j = offs[c] + before;
        for (uint32_t v = 0; v < wave; ++v) j += wave_count[v];
        __syncthreads();
        if (!cov || j >= cap) continue;
        uint64_t lo = 0, len = S;      // the first record with pos >= p
        while (len) {
            const uint64_t half = len >> 1;
            if (pos[lo + half] < p) lo += half + 1, len -= half + 1;
            else len = half;
        }
        uint64_t cnt = 0;               // the records from there on with first <= p: w at the most
        while (cnt < w && lo + cnt < S && first[lo + cnt] <= p) ++cnt;
        crow[j] = i;
        clo[j] = lo | (cnt << 56);
    }
}

__global__ __launch_bounds__(256) void k_mk_heads(const uint64_t *__restrict__ crow, const uint64_t *__restrict__ clo, const uint64_t *__restrict__ val,
                                                  const uint64_t C, uint64_t *__restrict__ hsum, uint64_t *__restrict__ vsum) {
    MK_FOR(j, C) {
        const uint64_t e = clo[j], cnt = e >> 56;
        bool head = true;
        if (j && cnt == 1) {
            const uint64_t pe = clo[j - 1];
            head = !(crow[j - 1] + 1 == crow[j] && (pe >> 56) == 1 && val[pe & kMkLoMask] == val[e & kMkLoMask]);
        }
        hsum[j] = head ? 1 : 0;
        vsum[j] = head ? cnt : 0;
    }
}

// ascending, by a bitonic network whose indices are all known when it is compiled: the values never leave the registers
template <int W>
__device__ __forceinline__ void mk_sort(uint64_t (&v)[W]) {
#pragma unroll
    for (int k = 2; k <= W; k *= 2) {
#pragma unroll
        for (int s = k / 2; s > 0; s /= 2) {
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const int l = i ^ s;
                if (l > i) {
                    const uint64_t a = v[i], b = v[l];
                    const bool swap = ((i & k) == 0) == (a > b);
                    v[i] = swap ? b : a;
                    v[l] = swap ? a : b;
                }
            }
        }
    }
}

// hsum, vsum: scanned (inclusive)
template <int W>
__global__ __launch_bounds__(256) void k_mk_fill(const uint64_t *__restrict__ crow, const uint64_t *__restrict__ clo, const uint64_t *__restrict__ hsum,
                                                 const uint64_t *__restrict__ vsum, const uint64_t *__restrict__ val, const uint64_t C, const uint64_t nruns,
                                                 const uint64_t nvals, uint64_t *__restrict__ run_start, uint64_t *__restrict__ run_end,
                                                 uint64_t *__restrict__ mk_off, uint64_t *__restrict__ mk_vals) {
    MK_FOR(j, C) {
        const uint64_t h = hsum[j], id = h - 1;
        if (id >= nruns) continue;      // (the counts are the plan's: checked on the host.  Nothing is written out of bounds whatever they are)
        const uint64_t row = crow[j];
        if (j + 1 == C || hsum[j + 1] != h) run_end[id] = row;
        if (j + 1 == C) mk_off[nruns] = nvals;
        if (j && hsum[j - 1] == h) continue;
        const uint64_t e = clo[j], cnt = e >> 56, lo = e & kMkLoMask, off = vsum[j] - cnt;
        run_start[id] = row;
        mk_off[id] = off;
        if (off + cnt > nvals) continue;
        if (cnt == 1) {
            mk_vals[off] = val[lo];
            continue;
        }
        uint64_t v[W];
#pragma unroll
        for (int k = 0; k < W; ++k) v[k] = static_cast<uint64_t>(k) < cnt ? val[lo + k] : ~0ull;
        mk_sort<W>(v);
#pragma unroll
        for (int k = 0; k < W; ++k)
            if (static_cast<uint64_t>(k) < cnt) mk_vals[off + k] = v[k];
    }
}

inline size_t mk_up256(const size_t b) { return (b + 255) & ~size_t(255); }

struct MkLayout {
    uint64_t nchunks, cap;
    size_t hdr, bits, bits_bytes, counts, counts_bytes, crow, clo, hsum, vsum, cub, cub_bytes, total;
};

MkLayout mk_layout(const uint64_t n, const uint64_t S, const uint32_t w) {
    MkLayout L{};
    L.nchunks = (n + kMkThreads - 1) / kMkThreads;
    L.cap = std::min<uint64_t>(n, S * w);      // (S <= n <= 2^56 and w <= 64: the product fits)
    const size_t list = mk_up256(static_cast<size_t>(L.cap) * 8);
    size_t at = 0;
    L.hdr = at, at += 256;
    L.bits = at, L.bits_bytes = mk_up256(static_cast<size_t>((n + 63) / 64) * 8), at += L.bits_bytes;
    L.counts = at, L.counts_bytes = mk_up256(static_cast<size_t>(L.nchunks + 1) * 8), at += L.counts_bytes;
    L.crow = at, at += list;
    L.clo = at, at += list;
    L.hsum = at, at += list;
    L.vsum = at, at += list;
    L.cub = at;
    size_t a = 0, b = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, a, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), static_cast<int64_t>(L.nchunks + 1));
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, b, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), static_cast<int64_t>(L.cap ? L.cap : 1));
    L.cub_bytes = mk_up256(std::max(a, b));
    L.total = at + L.cub_bytes;
    return L;
}

inline bool mk_args_ok(const uint64_t n, const uint64_t S, const uint32_t w) { return n != 0 && n <= (1ull << 56) && S <= n && w >= 1 && w <= 64; }

#define MK_HIP(expr)                                   \
    do {                                               \
        if ((expr) != hipSuccess) {                    \
            (void)hipGetLastError();                   \
            return 2;                                  \
        }                                              \
    } while (0)
#define MK_LAUNCH(expr)                                \
    do {                                               \
        if (expr) return 2;                            \
    } while (0)

}  // namespace

// 0 = arguments no plan takes
size_t marker_runs_tmp_bytes(uint64_t n, uint64_t S, uint32_t w) { return mk_args_ok(n, S, w) ? mk_layout(n, S, w).total : 0; }

// 0: done, *nruns and *nvals set; 1: the records break their rule (or arguments no plan takes); 2: a HIP error.  Waits for the stream
int marker_runs_plan(const void *sa, uint64_t n, uint32_t pos_bytes, const uint64_t *pos, const uint64_t *first, const uint64_t *val, uint64_t S, uint32_t w,
                     void *tmp, size_t tmp_bytes, uint64_t *nruns, uint64_t *nvals, void *stream) {
    if (!mk_args_ok(n, S, w)) return 1;
    const MkLayout L = mk_layout(n, S, w);
    if (tmp_bytes < L.total) return 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t *t = static_cast<uint8_t *>(tmp);
    MkHeader h{kMkMagic, n, S, static_cast<uint64_t>(w) | static_cast<uint64_t>(pos_bytes) << 32, 0, 0, 0, 0};
    MkHeader *d_hdr = reinterpret_cast<MkHeader *>(t + L.hdr);
    MK_HIP(hipMemsetAsync(d_hdr, 0, 256, st));      // (a plan that fails half-way leaves no header a fill would take)
    if (S) {
        const dim3 block(kMkThreads);
        unsigned long long *bits = reinterpret_cast<unsigned long long *>(t + L.bits);
        uint64_t *counts = reinterpret_cast<uint64_t *>(t + L.counts);
        uint64_t *crow = reinterpret_cast<uint64_t *>(t + L.crow), *clo = reinterpret_cast<uint64_t *>(t + L.clo);
        uint64_t *hsum = reinterpret_cast<uint64_t *>(t + L.hsum), *vsum = reinterpret_cast<uint64_t *>(t + L.vsum);
        MK_HIP(hipMemsetAsync(bits, 0, L.bits_bytes + L.counts_bytes, st));
        MK_LAUNCH(launch_grid(k_mk_cover, mk_grid(S), block, 0, st, pos, first, S, n, w, bits, reinterpret_cast<unsigned long long *>(&d_hdr->err)));
        const dim3 sweep(static_cast<uint32_t>(std::min(L.nchunks, kMkGridCap)));
        size_t cb = L.cub_bytes;
        const int rc = with_pos(pos_bytes, [&](auto p) -> int {
            using P = pos_t<decltype(p)>;
            MK_LAUNCH(launch_grid(k_mk_count<P>, sweep, block, 0, st, static_cast<const P *>(sa), static_cast<const unsigned long long *>(bits), n, L.nchunks,
                                  counts));
            MK_HIP(hipcub::DeviceScan::ExclusiveSum(t + L.cub, cb, counts, counts, static_cast<int64_t>(L.nchunks + 1), st));
            MK_LAUNCH(launch_grid(k_mk_compact<P>, sweep, block, 0, st, static_cast<const P *>(sa), static_cast<const unsigned long long *>(bits), n, L.nchunks,
                                  static_cast<const uint64_t *>(counts), pos, first, S, w, L.cap, crow, clo));
            return 0;
        });
        if (rc) return rc;
        uint64_t C = 0, err = 0;
        MK_HIP(hipMemcpyAsync(&C, counts + L.nchunks, 8, hipMemcpyDeviceToHost, st));
        MK_HIP(hipMemcpyAsync(&err, &d_hdr->err, 8, hipMemcpyDeviceToHost, st));
        MK_HIP(hipStreamSynchronize(st));
        if (err) return 1;
        if (C == 0 || C > L.cap) return 2;      // (every record covers its own position: S >= 1 gives a covered row)
        MK_LAUNCH(launch_grid(k_mk_heads, mk_grid(C), block, 0, st, static_cast<const uint64_t *>(crow), static_cast<const uint64_t *>(clo), val, C, hsum, vsum));
        cb = L.cub_bytes;
        MK_HIP(hipcub::DeviceScan::InclusiveSum(t + L.cub, cb, hsum, hsum, static_cast<int64_t>(C), st));
        cb = L.cub_bytes;
        MK_HIP(hipcub::DeviceScan::InclusiveSum(t + L.cub, cb, vsum, vsum, static_cast<int64_t>(C), st));
        MK_HIP(hipMemcpyAsync(&h.nruns, hsum + (C - 1), 8, hipMemcpyDeviceToHost, st));
        MK_HIP(hipMemcpyAsync(&h.nvals, vsum + (C - 1), 8, hipMemcpyDeviceToHost, st));
        MK_HIP(hipStreamSynchronize(st));
        h.C = C;
    }
    MK_HIP(hipMemcpyAsync(d_hdr, &h, sizeof h, hipMemcpyHostToDevice, st));
    MK_HIP(hipStreamSynchronize(st));
    *nruns = h.nruns;
    *nvals = h.nvals;
    return 0;
}

// 0: queued; 1: tmp does not hold the plan of these arguments and counts; 2: a HIP error.  Waits for what the stream holds (it reads the plan's header
// back), then queues its kernels and returns
int marker_runs_fill(uint64_t n, uint32_t pos_bytes, const uint64_t *val, uint64_t S, uint32_t w, const void *tmp, size_t tmp_bytes, uint64_t nruns,
                     uint64_t nvals, uint64_t *run_start, uint64_t *run_end, uint64_t *mk_off, uint64_t *mk_vals, void *stream) {
    if (!mk_args_ok(n, S, w)) return 1;
    const MkLayout L = mk_layout(n, S, w);
    if (tmp_bytes < L.total) return 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t *t = static_cast<const uint8_t *>(tmp);
    MkHeader h{};
    MK_HIP(hipMemcpyAsync(&h, t + L.hdr, sizeof h, hipMemcpyDeviceToHost, st));
    MK_HIP(hipStreamSynchronize(st));
    if (h.magic != kMkMagic || h.n != n || h.S != S || h.w_pb != (static_cast<uint64_t>(w) | static_cast<uint64_t>(pos_bytes) << 32) || h.err || h.C > L.cap ||
        h.nruns != nruns || h.nvals != nvals || nruns > h.C || (h.C != 0) != (S != 0))
        return 1;
    if (h.C == 0) {
        MK_HIP(hipMemsetAsync(mk_off, 0, 8, st));
        return 0;
    }
    const uint64_t *crow = reinterpret_cast<const uint64_t *>(t + L.crow), *clo = reinterpret_cast<const uint64_t *>(t + L.clo);
    const uint64_t *hsum = reinterpret_cast<const uint64_t *>(t + L.hsum), *vsum = reinterpret_cast<const uint64_t *>(t + L.vsum);
    auto go = [&](auto kern) -> int {
        MK_LAUNCH(launch_grid(kern, mk_grid(h.C), dim3(kMkThreads), 0, st, crow, clo, hsum, vsum, val, h.C, nruns, nvals, run_start, run_end, mk_off, mk_vals));
        return 0;
    };
    return w <= 4 ? go(k_mk_fill<4>) : w <= 16 ? go(k_mk_fill<16>) : go(k_mk_fill<64>);
}

}  // namespace rbg
