// k_sam.hip -- rbg_align_sam's device steps (include/rbg.h; the rules of the lines: rbg_sam.hpp).
//
//   k_sam_strands    N reads -> the 2N-sequence batch the *_dev searches take: sequence 2i = read i as given, 2i + 1 = its reverse complement under
//                    sam_comp (N stays N, unlike k_read_strands' seq_ntoa_table); off2[2N + 1] as launch_read_strands writes it
//   k_sam_pick       per read, from the 2N answers of launch_greedy_seed: the strand with the longer seed (a tie: forward; none: unmapped, range {1, 0});
//                    the read's lines: one, or its locations up to max_hits
//   k_sam_mark / max-scan / k_sam_len / exclusive sum / k_sam_write
//                    k_text.hip's structure with one element per output LINE: heads marked with their read, every line learns its read, lengths and the
//                    document of every location, offsets, and the text -- kSamLines lines per workgroup formatted into LDS at their offsets, the
//                    workgroup's stretch leaving in aligned 16-byte stores; a stretch longer than kSamLds goes straight to memory, lane by lane.
//                    SEQ and QUAL of a reverse-strand line are made here from the read's original bytes, never staged in memory.
//
// A SAM line is about name + 2 m + 40 bytes (240 at 100 bp, 340 at 150 bp), six times k_text.hip's elements, so a workgroup takes kSamLines = 128 lines
// (one lane each) and stages kSamLds = 48 KB: three workgroups fit gfx950's 160 KB of LDS per CU.
// Grids are capped (kSamGridCap workgroups, or the launcher's `cap` argument when it is not 0: rbg_align_sam reads RBG_SAM_GRID_CAP once per call) and every kernel strides over its work.
#include <hipcub/hipcub.hpp>

#include "rbg_sam_dev.hpp"   // the batch, the parts of a line and the write body, shared with sam_extend.hip

namespace rbg {
namespace {

constexpr uint32_t kSamLines = 128;        // lines per workgroup of k_sam_write (= its threads)
constexpr uint32_t kSamLds = 48 * 1024;    // bytes of text a workgroup stages

// One lane makes one aligned 16-byte piece of the output, cut where a strand ends (k_read_strands' layout; the source is read byte by byte)
__global__ __launch_bounds__(256) void k_sam_strands(const uint8_t *__restrict__ seqs, const uint64_t *__restrict__ off, const uint64_t N,
                                                     uint8_t *__restrict__ out, uint64_t *__restrict__ off2) {
    const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x, stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const uint64_t T = off[N];   // (off[0] == 0: the call packs the batch itself)
    for (uint64_t i = tid; i <= 2 * N; i += stride) {
        const uint64_t r = i >> 1;
        off2[i] = 2 * off[r] + ((i & 1) ? off[r + 1] - off[r] : 0);
    }
    const uint64_t nchunks = (2 * T + 15) >> 4;
    for (uint64_t c = tid; c < nchunks; c += stride) {
        uint64_t p = c << 4;
        const uint64_t end = p + 16 < 2 * T ? p + 16 : 2 * T;
        uint64_t lo = 0, hi = N - 1;   // the first read whose two strands end beyond p
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (2 * off[mid + 1] > p) hi = mid; else lo = mid + 1;
        }
        uint64_t i = lo;
        uint32_t w[4] = {0, 0, 0, 0};
        while (p < end) {
            const uint64_t o = off[i], len = off[i + 1] - o, b = 2 * o;
            if (p >= b + 2 * len) { ++i; continue; }
            const uint64_t r = p - b;
            const uint8_t ch = r < len ? seqs[o + r] : sam_comp(seqs[o + (2 * len - 1 - r)]);
            const uint32_t j = static_cast<uint32_t>(p & 15);
            w[j >> 2] |= static_cast<uint32_t>(ch) << ((j & 3) * 8);
            ++p;
        }
        reinterpret_cast<uint4 *>(out)[c] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

__global__ __launch_bounds__(256) void k_sam_pick(const uint64_t *__restrict__ lo2, const uint64_t *__restrict__ hi2, const uint64_t *__restrict__ qs2,
                                                  const uint64_t *__restrict__ qe2, const uint64_t *__restrict__ ss2, const uint64_t N, const uint64_t max_hits,
                                                  uint64_t *__restrict__ lo, uint64_t *__restrict__ hi, uint64_t *__restrict__ k, uint64_t *__restrict__ a,
                                                  uint64_t *__restrict__ b, uint8_t *__restrict__ rev, uint64_t *__restrict__ nlines,
                                                  unsigned long long *__restrict__ counters) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    // both strands of every read were searched (the seeding kernels do not count reads)
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&counters[0], static_cast<unsigned long long>(2 * N));
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i <= N; i += stride) {
        if (i == N) { nlines[N] = 0; continue; }   // (the scan runs over N + 1 entries: line_off[N] is the number of lines)
        const uint64_t f = 2 * i, r = f + 1;
        const uint64_t lf = hi2[f] >= lo2[f] ? qe2[f] - qs2[f] : 0, lr = hi2[r] >= lo2[r] ? qe2[r] - qs2[r] : 0;
        const uint64_t s = lr > lf ? r : f;
        const bool mapped = (lr > lf ? lr : lf) > 0;
        lo[i] = mapped ? lo2[s] : 1;
        hi[i] = mapped ? hi2[s] : 0;
        k[i] = mapped ? ss2[s] : 0;
        a[i] = mapped ? qs2[s] : 0;
        b[i] = mapped ? qe2[s] : 0;
        rev[i] = mapped && s == r ? 1 : 0;
        const uint64_t occ = mapped ? hi2[s] - lo2[s] + 1 : 1;
        nlines[i] = occ < max_hits ? occ : max_hits;   // (max_hits >= 1)
    }
}

__global__ __launch_bounds__(256) void k_sam_mark(const uint64_t *__restrict__ line_off, const uint64_t N, uint32_t *__restrict__ mark) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < N; i += stride) mark[line_off[i]] = static_cast<uint32_t>(i);
}

__global__ __launch_bounds__(256) void k_sam_len(const SamArgs s, const uint32_t *__restrict__ eread, uint64_t *__restrict__ len, uint32_t *__restrict__ doc,
                                                 unsigned int *__restrict__ bad) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < s.E; e += stride) {
        const uint64_t i = eread[e];
        uint32_t d = 0;
        if (s.hi[i] >= s.lo[i]) {
            const uint64_t j = sam_doc_of(s, s.locs[s.loc_off[i] + (e - s.line_off[i])]);
            if (j == 0) { atomicOr(bad, 1u); len[e] = 0; doc[e] = 0; continue; }
            d = static_cast<uint32_t>(j - 1);
        }
        doc[e] = d;
        len[e] = sam_line_len(sam_line_of(s, e, i, d));
    }
}

__global__ __launch_bounds__(kSamLines) void k_sam_write(const SamArgs s, const uint32_t *__restrict__ eread, const uint32_t *__restrict__ doc,
                                                         const uint64_t *__restrict__ at, const uint64_t total, char *__restrict__ text) {
    __shared__ __align__(16) char s_buf[kSamLds + 16];
    sam_write_lines<kSamLines, kSamLds>(s, eread, doc, at, total, text, s_buf, nullptr);
}

struct SamMaxOp {
    __device__ __forceinline__ uint32_t operator()(uint32_t x, uint32_t y) const { return x > y ? x : y; }
};

size_t sam_scan_bytes(uint64_t E) {
    size_t s1 = 0, s2 = 0;
    (void)hipcub::DeviceScan::InclusiveScan(nullptr, s1, static_cast<uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr), SamMaxOp(), static_cast<int64_t>(E ? E : 1));
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, s2, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), static_cast<int64_t>(E ? E : 1));
    return std::max(s1, s2);
}
SamWs sam_ws_of(void *ws, uint64_t E) {
    SamWs w = sam_ws_ptrs(ws, E);
    w.tmp_bytes = up256(sam_scan_bytes(E));
    return w;
}

}  // namespace

int launch_sam_strands(const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t total, uint8_t *out, uint64_t *off2, uint32_t cap, void *stream) {
    hipLaunchKernelGGL(k_sam_strands, dim3(sam_grid(std::max<uint64_t>((2 * total + 15) / 16, 2 * N + 1), 256, cap)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       seqs, off, N, out, off2);
    return static_cast<int>(hipGetLastError());
}

size_t sam_pick_tmp_bytes(uint64_t N) {
    size_t s = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, s, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), static_cast<int64_t>(N + 1));
    return up256(s);
}
// nlines / line_off: [N + 1] each; line_off[N] = the number of lines
int launch_sam_pick(const uint64_t *lo2, const uint64_t *hi2, const uint64_t *qs2, const uint64_t *qe2, const uint64_t *ss2, uint64_t N, uint64_t max_hits,
                    uint64_t *lo, uint64_t *hi, uint64_t *k, uint64_t *a, uint64_t *b, uint8_t *rev, uint64_t *nlines, uint64_t *line_off,
                    unsigned long long *counters, void *tmp, size_t tmp_bytes, uint32_t cap, void *stream) {
    if (max_hits == 0 || tmp_bytes < sam_pick_tmp_bytes(N)) return static_cast<int>(hipErrorInvalidValue);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_sam_pick, dim3(sam_grid(N + 1, 256, cap)), dim3(256), 0, st, lo2, hi2, qs2, qe2, ss2, N, max_hits, lo, hi, k, a, b, rev, nlines, counters);
    size_t tb = tmp_bytes;
    // (tmp and the workspace of launch_sam_plan are the library's own allocations, 256-byte aligned: never a caller's pointer)
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum(tmp, tb, nlines, line_off, static_cast<int64_t>(N + 1), st);
    if (e != hipSuccess) return static_cast<int>(e);
    return static_cast<int>(hipGetLastError());
}

size_t sam_ws_bytes(uint64_t E) { return 2 * up256(E * 4) + 2 * up256(E * 8) + up256(sam_scan_bytes(E)) + 1024; }

// phase 1: every line's read, length, document and offset.  *d_bad != 0: a location before every document
int launch_sam_plan(const SamBatch &B, void *ws, size_t ws_bytes, unsigned int *d_bad, uint32_t cap, void *stream) {
    if (ws_bytes < sam_ws_bytes(B.E) || (reinterpret_cast<uintptr_t>(ws) & 255)) return static_cast<int>(hipErrorInvalidValue);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SamWs w = sam_ws_of(ws, B.E);
    const SamArgs s = sam_args(B);
    hipError_t e = hipMemsetAsync(w.eread, 0, B.E * 4, st);
    if (e != hipSuccess) return static_cast<int>(e);
    hipLaunchKernelGGL(k_sam_mark, dim3(sam_grid(B.N, 256, cap)), dim3(256), 0, st, B.line_off, B.N, w.eread);
    size_t tb = w.tmp_bytes;
    e = hipcub::DeviceScan::InclusiveScan(w.tmp, tb, w.eread, w.eread, SamMaxOp(), static_cast<int64_t>(B.E), st);
    if (e != hipSuccess) return static_cast<int>(e);
    hipLaunchKernelGGL(k_sam_len, dim3(sam_grid(B.E, 256, cap)), dim3(256), 0, st, s, w.eread, w.len, w.doc, d_bad);
    tb = w.tmp_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(w.tmp, tb, w.len, w.at, static_cast<int64_t>(B.E), st);
    if (e != hipSuccess) return static_cast<int>(e);
    return static_cast<int>(hipGetLastError());
}
// the second half of the plan alone: every line's offset from the lengths already in the workspace (sam_extend.hip writes them with its own kernel)
int launch_sam_offsets(void *ws, uint64_t E, void *stream) {
    const SamWs w = sam_ws_of(ws, E);
    size_t tb = w.tmp_bytes;
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum(w.tmp, tb, w.len, w.at, static_cast<int64_t>(E), static_cast<hipStream_t>(stream));
    return static_cast<int>(e != hipSuccess ? e : hipGetLastError());
}
// where the total is: at[E - 1] + len[E - 1]
void sam_total_ptrs(void *ws, uint64_t E, const uint64_t **last_at, const uint64_t **last_len) {
    const SamWs w = sam_ws_of(ws, E);
    *last_at = w.at + (E - 1);
    *last_len = w.len + (E - 1);
}
// phase 2: the text (total bytes at `text`)
int launch_sam_fill(const SamBatch &B, void *ws, uint64_t total, char *text, uint32_t cap, void *stream) {
    const SamWs w = sam_ws_of(ws, B.E);
    hipLaunchKernelGGL(k_sam_write, dim3(sam_grid(B.E, kSamLines, cap)), dim3(kSamLines), 0, static_cast<hipStream_t>(stream), sam_args(B), w.eread, w.doc, w.at,
                       total, text);
    return static_cast<int>(hipGetLastError());
}

}  // namespace rbg
