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

#include "rbg_device.hpp"
#include "rbg_sam.hpp"

namespace rbg {
namespace {

constexpr uint32_t kSamLines = 128;        // lines per workgroup of k_sam_write (= its threads)
constexpr uint32_t kSamLds = 48 * 1024;    // bytes of text a workgroup stages
constexpr uint32_t kSamGridCap = 4096;     // workgroups per launch, at most

struct SamArgs {
    uint64_t N, E;                                  // reads, lines
    const uint64_t *lo, *hi, *a, *b;                // [N] the picked seed (unmapped: lo = 1, hi = 0)
    const uint8_t *rev;                             // [N]
    const uint64_t *line_off, *loc_off, *locs;      // [N + 1], [N + 1], [loc_off[N]]
    const char *seqs, *quals;                       // the reads' original bytes; quals nullable, same offsets
    const uint64_t *roff;                           // [N + 1]
    const char *names;
    const uint32_t *name_off;                       // [N + 1]
    const uint64_t *doc_start;                      // [ndocs] sorted
    const char *doc_names;
    const uint32_t *doc_name_off;                   // [ndocs + 1]
    uint64_t ndocs, text_size;
};

int sam_grid(const uint64_t work, const uint32_t per_block, const uint32_t cap_arg) {
    const uint64_t cap = cap_arg ? cap_arg : kSamGridCap;
    const uint64_t g = (work + per_block - 1) / per_block;
    return static_cast<int>(std::max<uint64_t>(1, std::min(g, cap)));
}

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

// k_text.hip's doc_of: the number of sorted starts below min(pos + 1, size); 0: no document
__device__ __forceinline__ uint64_t sam_doc_of(const SamArgs &s, const uint64_t pos) {
    const uint64_t q = pos + 1 > s.text_size ? s.text_size : pos + 1;
    uint64_t lo = 0, hi = s.ndocs;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (s.doc_start[mid] < q) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the parts of line e of read i (d: its document, for a mapped line)
__device__ __forceinline__ SamLine sam_line_of(const SamArgs &s, const uint64_t e, const uint64_t i, const uint32_t d) {
    SamLine L;
    L.name_len = s.name_off[i + 1] - s.name_off[i];
    L.mapped = s.hi[i] >= s.lo[i];
    L.reverse = s.rev[i] != 0;
    L.hit = e - s.line_off[i] + 1;
    L.occ = s.hi[i] - s.lo[i] + 1;
    L.m = s.roff[i + 1] - s.roff[i];
    L.a = s.a[i];
    L.b = s.b[i];
    L.has_qual = s.quals != nullptr;
    L.rname_len = 0;
    L.pos = 0;
    if (L.mapped) {
        const uint64_t pos = s.locs[s.loc_off[i] + (L.hit - 1)];
        L.rname_len = s.doc_name_off[d + 1] - s.doc_name_off[d];
        L.pos = pos - s.doc_start[d] + 1;
    }
    return L;
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

__device__ __forceinline__ void sam_put(const SamArgs &s, const uint64_t e, const uint64_t i, const uint32_t d, char *p) {
    const SamLine L = sam_line_of(s, e, i, d);
    sam_put_line(p, L, s.names + s.name_off[i], s.doc_names + s.doc_name_off[d], s.seqs + s.roff[i], s.quals ? s.quals + s.roff[i] : nullptr);
}

__global__ __launch_bounds__(kSamLines) void k_sam_write(const SamArgs s, const uint32_t *__restrict__ eread, const uint32_t *__restrict__ doc,
                                                         const uint64_t *__restrict__ at, const uint64_t total, char *__restrict__ text) {
    __shared__ __align__(16) char s_buf[kSamLds + 16];
    const uint64_t nblocks = (s.E + kSamLines - 1) / kSamLines;
    for (uint64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const uint64_t e0 = blk * kSamLines, e1 = e0 + kSamLines < s.E ? e0 + kSamLines : s.E;
        const uint64_t t0 = at[e0], t1 = e1 < s.E ? at[e1] : total;
        const uint64_t e = e0 + threadIdx.x;
        const uint32_t shift = static_cast<uint32_t>((reinterpret_cast<uintptr_t>(text) + t0) & 15u);   // LDS and memory addresses congruent mod 16
        if (t1 - t0 <= kSamLds) {
            if (e < e1) sam_put(s, e, eread[e], doc[e], s_buf + shift + (at[e] - t0));
            __syncthreads();
            const uint32_t nbytes = static_cast<uint32_t>(t1 - t0);
            char *dst = text + t0;
            const char *src = s_buf + shift;
            const uint32_t head = (16u - shift) & 15u;                      // bytes before the first 16-byte boundary
            const uint32_t h = head < nbytes ? head : nbytes;
            if (threadIdx.x < h) dst[threadIdx.x] = src[threadIdx.x];
            const uint32_t body = (nbytes - h) >> 4;
            for (uint32_t j = threadIdx.x; j < body; j += kSamLines)
                reinterpret_cast<uint4 *>(dst + h)[j] = reinterpret_cast<const uint4 *>(src + h)[j];
            const uint32_t done = h + (body << 4);
            if (threadIdx.x < nbytes - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
            __syncthreads();
        } else if (e < e1) {
            sam_put(s, e, eread[e], doc[e], text + at[e]);                  // (a long name or read: straight to memory, byte by byte)
        }
    }
}

struct SamMaxOp {
    __device__ __forceinline__ uint32_t operator()(uint32_t x, uint32_t y) const { return x > y ? x : y; }
};

size_t up256(size_t x) { return (x + 255) & ~size_t(255); }
// the workspace: eread / doc (4 bytes per line), len / at (8), the scans' temporaries
struct SamWs {
    uint32_t *eread, *doc;
    uint64_t *len, *at;
    void *tmp;
    size_t tmp_bytes;
};
size_t sam_scan_bytes(uint64_t E) {
    size_t s1 = 0, s2 = 0;
    (void)hipcub::DeviceScan::InclusiveScan(nullptr, s1, static_cast<uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr), SamMaxOp(), static_cast<int64_t>(E ? E : 1));
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, s2, static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), static_cast<int64_t>(E ? E : 1));
    return std::max(s1, s2);
}
SamWs sam_ws_of(void *ws, uint64_t E) {
    char *b = static_cast<char *>(ws);
    SamWs w;
    w.eread = reinterpret_cast<uint32_t *>(b);
    w.doc = reinterpret_cast<uint32_t *>(b + up256(E * 4));
    w.len = reinterpret_cast<uint64_t *>(b + 2 * up256(E * 4));
    w.at = reinterpret_cast<uint64_t *>(b + 2 * up256(E * 4) + up256(E * 8));
    w.tmp = b + 2 * up256(E * 4) + 2 * up256(E * 8);
    w.tmp_bytes = up256(sam_scan_bytes(E));
    return w;
}

SamArgs sam_args(const SamBatch &B) {
    return SamArgs{B.N, B.E, B.lo, B.hi, B.a, B.b, B.rev, B.line_off, B.loc_off, B.locs, B.seqs, B.quals, B.roff, B.names, B.name_off,
                   B.doc_start, B.doc_names, B.doc_name_off, B.ndocs, B.text_size};
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
