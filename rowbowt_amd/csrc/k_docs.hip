// k_docs.hip -- which documents a read's locations fall in (rbg_doc_hits_dev, rbg_resolve_offsets_dev; include/rbg.h).  Input is what K3 leaves on the
// device: locs (64-bit, or the 32-bit form of rbg_locate_fill_dev32) and loc_off[N + 1].  The lookup is rbg_docdir.hpp's doc_rank -- DocList::doc_and_offset_at,
// doclist.hpp:46-50, over doc_bounds_rank, :77-79 -- the same text the host compiles.
//
// k_resolve_offsets: one location per lane, grid-stride: its document (kDocNone: none) and, optionally, its offset.
// k_doc_hits, per read: the SET of documents among its locations as W = ceil(ndocs / 64) u64 words, the number of distinct documents, the number of
// locations without a document, and +1 for every document of the set in doc_reads[ndocs] (reads per document; a read counts once per document).
//
// PARTITION (as k_loc_markers.hip).  A group of G lanes (4, 16 or 64) owns one read and strides over its locations, which are contiguous: the loads coalesce.
// G is chosen ON THE DEVICE from loc_off[N] / N (doc_group_for), which the host does not have without a synchronisation the _dev calls never make; one
// kernel holds the three widths and branches on a value every lane agrees on.  RBG_DOCS_GROUP (4 / 16 / 64) forces one for tests and A/Bs.  The outputs
// are sets and sums of integers: they do not depend on G, on the grid or on the order in which the atomics arrive.
// THE SET of the read in flight lives in LDS, one per group, as 2 W words of 32 BITS (a u64 word in memory is two of them: the bit of document d is
// 1u << (d & 31) of word d >> 5 -- a 32-bit shift; a per-lane 64-bit shift by a variable amount is what DESIGN.md 2c keeps out of kernels).  It is filled
// with LDS atomic ORs and leaves as whole u64 stores; no global atomic per location.
// doc_reads is counted per WORKGROUP in LDS and leaves with one global atomicAdd per document that workgroup met, at its end.
// THE TABLE (sorted starts, directory) is staged in LDS while ndocs <= kDocLdsDocs.  Above that (up to kDocMaxDocs) the lookups read it from global memory,
// the sets alone stay in LDS -- 2 W words are then up to 8 KB, so groups are 64 lanes wide whatever the mean, four sets per workgroup -- and the histogram
// takes a global atomicAdd per read and document: slower, exact.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "rbg_dev.h"
#include "rbg_docdir.hpp"

namespace rbg {
namespace {

constexpr uint32_t kDocLdsDocs = 1024;
constexpr uint32_t kDocBlock = 256;          // lanes per workgroup of both kernels
constexpr uint32_t kDocMaxBlocks = 2048;     // the largest grid: eight workgroups for each of the 256 CUs; the loops stride beyond it
// the group width for a mean of L / N locations per read: 4 lanes up to kDocGroup4Mean, 16 up to kDocGroup16Mean, 64 beyond.  A location costs a lookup and
// an LDS atomic, a read costs the clearing, the flush and two reductions of its group whatever its length, and a wave of narrow groups pays that for sixteen
// reads at once: on the bench index (37 locations per read) 4 lanes take half the time of 16 and a fifth of 64 (profiles/doc_hits_rate.txt).
// The wider groups are for batches of long location lists, where few reads have to fill the device; those thresholds are not measured.
constexpr uint32_t kDocGroup4Mean = 64;
constexpr uint32_t kDocGroup16Mean = 512;

__device__ __forceinline__ int doc_group_for(const uint64_t L, const uint64_t N) {
    if (L <= kDocGroup4Mean * N) return 4;
    if (L <= kDocGroup16Mean * N) return 16;
    return 64;
}

// the table as a kernel sees it; dir has ndir = buckets + 1 entries
struct DocTab {
    const uint64_t *sorted;
    const uint32_t *dir;
    uint64_t size;
    uint32_t ndocs, shift, ndir;
};

// a location as the 64-bit position it stands for: 0xFFFFFFFF of the 32-bit form is the toehold that wrapped below zero (rbg_locate_fill_dev32)
__device__ __forceinline__ uint64_t widen(const uint64_t v) { return v; }
__device__ __forceinline__ uint64_t widen(const uint32_t v) { return v == 0xFFFFFFFFu ? ~uint64_t(0) : static_cast<uint64_t>(v); }

// LDS operations of one wave execute in issue order; this only stops the compiler from moving one lane's reads of a set above the other lanes' writes
// (and the other way round): a group lies within one wave
__device__ __forceinline__ void group_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int G>
__device__ __forceinline__ uint32_t group_sum32(uint32_t v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
    return v;
}

template <typename L>
__global__ __launch_bounds__(kDocBlock) void k_resolve_offsets(const DocTab t, const L *__restrict__ locs, const uint64_t M, uint32_t *__restrict__ doc,
                                                              uint64_t *__restrict__ offset) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < M; j += stride) {
        uint64_t o;
        doc[j] = doc_and_offset(t.sorted, t.dir, t.size, t.shift, widen(locs[j]), &o);
        if (offset) offset[j] = o;
    }
}

// every bit of a 32-bit set word -> the histogram.  (Sharing a word's bits out among the group's lanes was tried: it halves the time of 64-lane groups and
// costs the 4-lane groups a quarter on the bench index, and the 4-lane groups are the ones that index runs with.)
__device__ __forceinline__ void count_docs(uint32_t v, const uint32_t first, unsigned long long *hist) {
    while (v) {
        const uint32_t d = first + static_cast<uint32_t>(__builtin_ctz(v));
        v &= v - 1;
        atomicAdd(&hist[d], 1ull);   // the workgroup's counts in LDS, or doc_reads itself (tables above kDocLdsDocs)
    }
}

// sorted / dir: the table (LDS or global); set: this group's 2 W words in LDS; hist: the workgroup's counts in LDS (LDS) or doc_reads (nullable in both)
template <typename L, int G, bool LDS>
__device__ __forceinline__ void doc_hits_groups(const uint64_t *sorted, const uint32_t *dir, const uint64_t size, const uint32_t shift, const uint32_t W,
                                                uint32_t *set_base, unsigned long long *hist, const L *__restrict__ locs, const uint64_t *__restrict__ loc_off,
                                                const uint64_t N, uint64_t *__restrict__ sets, uint32_t *__restrict__ ndocs_out, uint32_t *__restrict__ nodoc_out) {
    const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t groups = static_cast<uint64_t>(gridDim.x) * blockDim.x / G;
    const uint32_t g = threadIdx.x & (G - 1);
    const uint32_t W32 = 2 * W;
    uint32_t *set = set_base + (threadIdx.x / G) * W32;
    for (uint64_t i = tid / G; i < N; i += groups) {
        for (uint32_t w = g; w < W32; w += G) set[w] = 0;
        group_lds_sync();
        const uint64_t e = loc_off[i + 1];
        uint32_t miss = 0;
        for (uint64_t j = loc_off[i] + g; j < e; j += G) {
            const uint32_t r = doc_rank(sorted, dir, size, shift, widen(locs[j]));
            if (r == 0) { ++miss; continue; }
            const uint32_t d = r - 1;
            atomicOr(&set[d >> 5], 1u << (d & 31));
        }
        group_lds_sync();
        uint32_t cnt = 0;
        for (uint32_t w = g; w < W; w += G) {
            const uint32_t lo = set[2 * w], hi = set[2 * w + 1];
            cnt += static_cast<uint32_t>(__builtin_popcount(lo) + __builtin_popcount(hi));
            if (sets) sets[i * W + w] = static_cast<uint64_t>(lo) | (static_cast<uint64_t>(hi) << 32);
            if (hist) {
                count_docs(lo, 64 * w, hist);
                count_docs(hi, 64 * w + 32, hist);
            }
        }
        cnt = group_sum32<G>(cnt);
        miss = group_sum32<G>(miss);
        if (g == 0) {
            if (ndocs_out) ndocs_out[i] = cnt;
            if (nodoc_out) nodoc_out[i] = miss;
        }
        group_lds_sync();   // (the words are read before the next read clears them)
    }
}

extern __shared__ unsigned long long doc_lds[];

// LDS of a workgroup, in 8-byte units first: sorted[ndocs] | hist[ndocs] | then 4-byte units: dir[ndir] | sets[(kDocBlock / 4) * 2 W]
inline size_t doc_hits_lds_bytes(const uint32_t ndocs, const uint32_t ndir, const uint32_t W) {
    return static_cast<size_t>(ndocs) * 16 + static_cast<size_t>(ndir) * 4 + static_cast<size_t>(kDocBlock / 4) * 2 * W * 4;
}
// LAUNCH BOUNDS: 256 threads; tools/kernel_resources.py lists registers and scratch (none).  The dynamic LDS is what the table needs.
template <typename L>
__global__ __launch_bounds__(kDocBlock) void k_doc_hits(const DocTab t, const L *__restrict__ locs, const uint64_t *__restrict__ loc_off, const uint64_t N,
                                                       uint64_t *__restrict__ sets, uint32_t *__restrict__ ndocs_out, uint32_t *__restrict__ nodoc_out,
                                                       unsigned long long *__restrict__ doc_reads, const int group) {
    unsigned long long *l_sorted = doc_lds;
    unsigned long long *l_hist = doc_lds + t.ndocs;
    uint32_t *l_dir = reinterpret_cast<uint32_t *>(doc_lds + 2 * static_cast<size_t>(t.ndocs));
    uint32_t *l_sets = l_dir + t.ndir;
    for (uint32_t k = threadIdx.x; k < t.ndocs; k += kDocBlock) { l_sorted[k] = t.sorted[k]; l_hist[k] = 0; }
    for (uint32_t k = threadIdx.x; k < t.ndir; k += kDocBlock) l_dir[k] = t.dir[k];
    __syncthreads();
    const uint32_t W = (t.ndocs + 63) / 64;
    const uint64_t *sorted = reinterpret_cast<const uint64_t *>(l_sorted);
    unsigned long long *hist = doc_reads ? l_hist : nullptr;
    const int G = group ? group : doc_group_for(loc_off[N], N);
    if (G == 4) doc_hits_groups<L, 4, true>(sorted, l_dir, t.size, t.shift, W, l_sets, hist, locs, loc_off, N, sets, ndocs_out, nodoc_out);
    else if (G == 16) doc_hits_groups<L, 16, true>(sorted, l_dir, t.size, t.shift, W, l_sets, hist, locs, loc_off, N, sets, ndocs_out, nodoc_out);
    else doc_hits_groups<L, 64, true>(sorted, l_dir, t.size, t.shift, W, l_sets, hist, locs, loc_off, N, sets, ndocs_out, nodoc_out);
    if (!doc_reads) return;   // (the same for every lane)
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < t.ndocs; k += kDocBlock) {
        const unsigned long long c = l_hist[k];
        if (c) atomicAdd(&doc_reads[k], c);
    }
}

// tables above kDocLdsDocs: the table in global memory, the sets of the workgroup's four 64-lane groups in LDS ((kDocBlock / 64) * 2 W words)
template <typename L>
__global__ __launch_bounds__(kDocBlock) void k_doc_hits_wide(const DocTab t, const L *__restrict__ locs, const uint64_t *__restrict__ loc_off, const uint64_t N,
                                                            uint64_t *__restrict__ sets, uint32_t *__restrict__ ndocs_out, uint32_t *__restrict__ nodoc_out,
                                                            unsigned long long *__restrict__ doc_reads) {
    const uint32_t W = (t.ndocs + 63) / 64;
    doc_hits_groups<L, 64, false>(t.sorted, t.dir, t.size, t.shift, W, reinterpret_cast<uint32_t *>(doc_lds), doc_reads, locs, loc_off, N, sets, ndocs_out,
                                  nodoc_out);
}

// locations per document from stored locations (the two-step path of rbg_doc_hits_locs): one location per lane, grid-stride, the table read from global
// memory as in k_resolve_offsets; the counts per workgroup in LDS while ndocs <= kDocLdsDocs (launched with ndocs * 8 bytes), global atomics above
template <typename L>
__global__ __launch_bounds__(kDocBlock) void k_doc_locs(const DocTab t, const L *__restrict__ locs, const uint64_t M, unsigned long long *__restrict__ doc_locs) {
    const bool lds = t.ndocs <= kDocLdsDocs;   // (the same for every lane)
    if (lds) {
        for (uint32_t k = threadIdx.x; k < t.ndocs; k += kDocBlock) doc_lds[k] = 0;
        __syncthreads();
    }
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < M; j += stride) {
        const uint32_t r = doc_rank(t.sorted, t.dir, t.size, t.shift, widen(locs[j]));
        if (r) atomicAdd(lds ? &doc_lds[r - 1] : &doc_locs[r - 1], 1ull);
    }
    if (!lds) return;
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < t.ndocs; k += kDocBlock) {
        const unsigned long long c = doc_lds[k];
        if (c) atomicAdd(&doc_locs[k], c);
    }
}

inline int doc_grid(const uint64_t lanes) {
    const uint64_t blocks = (lanes + kDocBlock - 1) / kDocBlock;
    return static_cast<int>(blocks > kDocMaxBlocks ? kDocMaxBlocks : (blocks ? blocks : 1));
}

template <typename L>
int resolve_offsets_launch(const DocTab &t, const L *locs, uint64_t M, uint32_t *doc, uint64_t *offset, hipStream_t st) {
    if (M == 0) return 0;
    hipLaunchKernelGGL(k_resolve_offsets<L>, dim3(doc_grid(M)), dim3(kDocBlock), 0, st, t, locs, M, doc, offset);
    return static_cast<int>(hipGetLastError());
}

template <typename L>
int doc_hits_launch(const DocTab &t, const L *locs, const uint64_t *loc_off, uint64_t N, uint64_t *sets, uint32_t *ndocs_out, uint32_t *nodoc_out,
                    uint64_t *doc_reads, int group, hipStream_t st) {
    if (N == 0) return 0;
    const uint32_t W = (t.ndocs + 63) / 64;
    unsigned long long *dr = reinterpret_cast<unsigned long long *>(doc_reads);
    if (t.ndocs > kDocLdsDocs) {
        const size_t lds = static_cast<size_t>(kDocBlock / 64) * 2 * W * 4;
        const uint64_t lanes = N > (~uint64_t(0)) / 64 ? ~uint64_t(0) : N * 64;
        hipLaunchKernelGGL(k_doc_hits_wide<L>, dim3(doc_grid(lanes)), dim3(kDocBlock), lds, st, t, locs, loc_off, N, sets, ndocs_out, nodoc_out, dr);
        return static_cast<int>(hipGetLastError());
    }
    // the grid for the widest group: a narrower one finds more groups in the same threads (the loops stride by the groups there are)
    const uint64_t w = group ? static_cast<uint64_t>(group) : 64u;
    const uint64_t lanes = N > (~uint64_t(0)) / w ? ~uint64_t(0) : N * w;
    hipLaunchKernelGGL(k_doc_hits<L>, dim3(doc_grid(lanes)), dim3(kDocBlock), doc_hits_lds_bytes(t.ndocs, t.ndir, W), st, t, locs, loc_off, N, sets, ndocs_out,
                       nodoc_out, dr, group);
    return static_cast<int>(hipGetLastError());
}

inline DocTab doc_tab(const uint64_t *sorted, const uint32_t *dir, uint64_t size, uint32_t ndocs, uint32_t shift, uint32_t ndir) {
    DocTab t;
    t.sorted = sorted; t.dir = dir; t.size = size; t.ndocs = ndocs; t.shift = shift; t.ndir = ndir;
    return t;
}

}  // namespace

int docs_group() {
    const char *e = std::getenv("RBG_DOCS_GROUP");
    if (!e || !*e) return 0;
    const int g = std::atoi(e);
    return g == 4 || g == 16 || g == 64 ? g : 0;
}

int launch_resolve_offsets(const uint64_t *sorted, const uint32_t *dir, uint64_t size, uint32_t ndocs, uint32_t shift, uint32_t ndir, const void *locs,
                           bool locs32, uint64_t M, uint32_t *doc, uint64_t *offset, void *stream) {
    const DocTab t = doc_tab(sorted, dir, size, ndocs, shift, ndir);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return locs32 ? resolve_offsets_launch(t, static_cast<const uint32_t *>(locs), M, doc, offset, st)
                  : resolve_offsets_launch(t, static_cast<const uint64_t *>(locs), M, doc, offset, st);
}

int launch_doc_locs(const uint64_t *sorted, const uint32_t *dir, uint64_t size, uint32_t ndocs, uint32_t shift, uint32_t ndir, const void *locs, bool locs32,
                    uint64_t M, uint64_t *doc_locs, void *stream) {
    if (M == 0) return 0;
    const DocTab t = doc_tab(sorted, dir, size, ndocs, shift, ndir);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t lds = ndocs <= kDocLdsDocs ? static_cast<size_t>(ndocs) * 8 : 0;
    unsigned long long *dl = reinterpret_cast<unsigned long long *>(doc_locs);
    if (locs32) hipLaunchKernelGGL(k_doc_locs<uint32_t>, dim3(doc_grid(M)), dim3(kDocBlock), lds, st, t, static_cast<const uint32_t *>(locs), M, dl);
    else hipLaunchKernelGGL(k_doc_locs<uint64_t>, dim3(doc_grid(M)), dim3(kDocBlock), lds, st, t, static_cast<const uint64_t *>(locs), M, dl);
    return static_cast<int>(hipGetLastError());
}

int launch_doc_hits(const uint64_t *sorted, const uint32_t *dir, uint64_t size, uint32_t ndocs, uint32_t shift, uint32_t ndir, const void *locs, bool locs32,
                    const uint64_t *loc_off, uint64_t N, uint64_t *sets, uint32_t *ndocs_out, uint32_t *nodoc_out, uint64_t *doc_reads, int group,
                    void *stream) {
    const DocTab t = doc_tab(sorted, dir, size, ndocs, shift, ndir);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return locs32 ? doc_hits_launch(t, static_cast<const uint32_t *>(locs), loc_off, N, sets, ndocs_out, nodoc_out, doc_reads, group, st)
                  : doc_hits_launch(t, static_cast<const uint64_t *>(locs), loc_off, N, sets, ndocs_out, nodoc_out, doc_reads, group, st);
}

}  // namespace rbg
