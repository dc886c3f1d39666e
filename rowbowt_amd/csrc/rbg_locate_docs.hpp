// rbg_locate_docs.hpp -- document hits from the phi walk itself (rbg_locate_doc_hits_dev; include/rbg.h): K3's chains (ToeholdSA::locate_range,
// toehold_sa.hpp:37-49) with every position resolved to its document as it is produced (rbg_docdir.hpp doc_rank: doclist.hpp:46-50 over :77-79) and
// nothing stored per location.  What k_locate_fill / k_locate_fill_runs2 stage and flush (ChainStage) and k_doc_hits reads back is replaced by this
// file; the phi step of each layout stays where it is and comes in as `phi`, the one the fill kernels' walk takes (k_locate.hip slot_phi, rbg_runs2_device.hpp run_phi).
//
// ONE LANE PER CHAIN, as in K3: the chain is serial, the reads are not; a wave waits for its longest chain.  Nothing crosses lanes inside a chain, so
// the lanes loop over their own counts.
// THE SET of the chain in flight is 2 W words of 32 bits in LDS (W = ceil(ndocs / 64); k_docs.hip: why 32), word w of lane l at [w * kLocDocBlock + l]:
// the lanes of a wave hit different banks for the same word.  A lane sets bits by plain read-modify-write of its own words; no atomic.
// nodoc and the count are registers.  At the end of the chain the lane stores its W u64 words, their popcount and nodoc, and adds 1 per set bit to the
// workgroup's doc_reads histogram in LDS (k_docs.hip count_docs).  LOCS = the instantiation that also counts LOCATIONS per document (doc_locs), one
// LDS atomic per location; a caller without doc_locs runs the other one.  Both histograms leave with one global atomicAdd per document the
// workgroup met.
// THE TABLE (sorted starts, directory) is staged in LDS as k_doc_hits stages it; the launch refuses tables above kLocDocLdsDocs (rbg_dev.h; the caller keeps
// the two-step path there).  The full 64-bit position is at hand: 2^64 - 1 (a toehold that wrapped below zero) has no document by the rule itself.
// ORDER (the workspace of launch_locate_order): lane j takes read order[j] and decodes its toehold from the sorted keys as the fill kernels
// do (rbg_chain_walk.hpp chain_toehold); the count is min(hi - lo + 1, max_hits) from lo[i], hi[i] -- there is no loc_off in this path, so no plan.
// ix.counters[3] grows by the positions walked, as in K3.
#pragma once

#include <mutex>

#include "rbg_chain_walk.hpp"
#include "rbg_docdir.hpp"
#include "rbg_runs_device.hpp"

namespace rbg {
namespace {

constexpr uint32_t kLocDocBlock = 256;         // lanes (chains in flight) per workgroup
constexpr uint32_t kLocDocMaxBlocks = 2048;    // the largest grid: eight workgroups for each of the 256 CUs; the loop strides beyond it

// LDS of a workgroup, 8-byte units first: sorted[ndocs] | reads[ndocs] | (LOCS) locs[ndocs] | then 4-byte units: dir[ndir] | sets[2 W][kLocDocBlock].
// At 1024 documents: 8 + 8 (+ 8) KB, 8 KB of directory, 32 KB of sets.
inline size_t locate_docs_lds_bytes(const uint32_t ndocs, const uint32_t ndir, const bool locs) {
    const uint32_t W = (ndocs + 63) / 64;
    return static_cast<size_t>(ndocs) * (locs ? 24 : 16) + static_cast<size_t>(ndir) * 4 + static_cast<size_t>(2 * W) * kLocDocBlock * 4;
}
inline int locate_docs_grid(const uint64_t N) {
    const uint64_t blocks = (N + kLocDocBlock - 1) / kLocDocBlock;
    return static_cast<int>(blocks > kLocDocMaxBlocks ? kLocDocMaxBlocks : (blocks ? blocks : 1));
}

// every bit of a 32-bit set word -> the workgroup's histogram (k_docs.hip count_docs)
__device__ __forceinline__ void locate_docs_count(uint32_t v, const uint32_t first, unsigned long long *hist) {
    while (v) {
        const uint32_t d = first + static_cast<uint32_t>(__builtin_ctz(v));
        v &= v - 1;
        atomicAdd(&hist[d], 1ull);
    }
}

// the body of both kernels; lds = the workgroup's dynamic LDS (locate_docs_lds_bytes); phi(k, cost) = the position before k in the chain, as the fill
// kernels' walk takes it (rbg_chain_walk.hpp; this walk is not instrumented and drops the cost)
template <typename P, bool LOCS, typename Phi>
__device__ __forceinline__ void locate_docs_walk(const DevIndex &ix, const DocTable &t, unsigned long long *lds, const uint64_t *__restrict__ lo,
                                                 const uint64_t *__restrict__ hi, const uint64_t *__restrict__ k, const uint64_t N, const uint64_t max_hits,
                                                 const uint32_t *__restrict__ order, const uint64_t *__restrict__ skeys, uint64_t *__restrict__ sets,
                                                 uint32_t *__restrict__ ndocs_out, uint32_t *__restrict__ nodoc_out, unsigned long long *__restrict__ doc_reads,
                                                 unsigned long long *__restrict__ doc_locs, Phi phi) {
    unsigned long long *l_sorted = lds;
    unsigned long long *l_reads = lds + t.ndocs;
    unsigned long long *l_locs = lds + 2 * static_cast<size_t>(t.ndocs);   // (LOCS only)
    uint32_t *l_dir = reinterpret_cast<uint32_t *>(lds + (LOCS ? 3 : 2) * static_cast<size_t>(t.ndocs));
    uint32_t *set = l_dir + t.ndir + threadIdx.x;   // word w of this lane: set[w * kLocDocBlock]
    for (uint32_t j = threadIdx.x; j < t.ndocs; j += kLocDocBlock) {
        l_sorted[j] = t.sorted[j];
        l_reads[j] = 0;
        if (LOCS) l_locs[j] = 0;
    }
    for (uint32_t j = threadIdx.x; j < t.ndir; j += kLocDocBlock) l_dir[j] = t.dir[j];
    __syncthreads();
    const uint64_t *sorted = reinterpret_cast<const uint64_t *>(l_sorted);
    const uint32_t W = (t.ndocs + 63) / 64, W32 = 2 * W;
    unsigned long long *hist = doc_reads ? l_reads : nullptr;
    unsigned long long c_locs = 0, cost = 0;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kLocDocBlock;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kLocDocBlock + threadIdx.x; j < N; j += stride) {
        const uint64_t i = order ? order[j] : j;
        if (i >= N) continue;   // (a permutation never holds one)
        uint64_t k1 = skeys ? chain_toehold<P>(ix, skeys, k, i, j) : k[i];
        const uint64_t l = lo[i], h = hi[i];
        uint64_t occ = h >= l ? h - l + 1 : 0;   // toehold_sa.hpp:38-39
        if (occ > max_hits) occ = max_hits;
        for (uint32_t w = 0; w < W32; ++w) set[w * kLocDocBlock] = 0;
        uint32_t miss = 0;
        for (uint64_t s = 0; s < occ; ++s) {
            if (s) k1 = phi(k1, cost);   // every location but a read's first is phi of the one before (toehold_sa.hpp:44)
            const uint32_t r = doc_rank(sorted, l_dir, t.size, t.shift, k1);
            if (r == 0) { ++miss; continue; }
            const uint32_t d = r - 1;
            set[(d >> 5) * kLocDocBlock] |= 1u << (d & 31);
            if (LOCS) atomicAdd(&l_locs[d], 1ull);
        }
        c_locs += occ;
        uint32_t cnt = 0;
        for (uint32_t w = 0; w < W; ++w) {
            const uint32_t a = set[2 * w * kLocDocBlock], b = set[(2 * w + 1) * kLocDocBlock];
            cnt += static_cast<uint32_t>(__builtin_popcount(a) + __builtin_popcount(b));
            if (sets) sets[i * W + w] = static_cast<uint64_t>(a) | (static_cast<uint64_t>(b) << 32);
            if (hist) {
                locate_docs_count(a, 64 * w, hist);
                locate_docs_count(b, 64 * w + 32, hist);
            }
        }
        if (ndocs_out) ndocs_out[i] = cnt;
        if (nodoc_out) nodoc_out[i] = miss;
    }
    c_locs = wave_sum(c_locs);
    if ((threadIdx.x & (kWave - 1)) == 0 && c_locs) atomicAdd(&ix.counters[3], c_locs);
    if (!doc_reads && !LOCS) return;   // (the same for every lane)
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < t.ndocs; j += kLocDocBlock) {
        if (doc_reads) { const unsigned long long c = l_reads[j]; if (c) atomicAdd(&doc_reads[j], c); }
        if (LOCS) { const unsigned long long c = l_locs[j]; if (c) atomicAdd(&doc_locs[j], c); }
    }
}

}  // namespace
}  // namespace rbg
