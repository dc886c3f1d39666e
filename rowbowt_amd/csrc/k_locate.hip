// k_locate.hip -- K3: phi chains (ToeholdSA::locate_range, toehold_sa.hpp:37-49), their plan (counts + scan) and their order (radix sort of the toeholds)
#include <cstdlib>

#include "rbg_device.hpp"
#include "rbg_launch.hpp"
#include "rbg_chain_walk.hpp"
#include "rbg_locate_docs.hpp"

namespace rbg {
namespace {

// ---- K3: locate (the counts of the plan are computed where its scan reads them: OccOf below) ---------
// ---- the locus order's sort key (rbg_dev.h order_docs): k <-> {offset >> low, document, offset & (2^low - 1)} -----------------------------
// A toehold outside the text (it wrapped below zero: k >= n) has no document: its key is all ones and K3 reads the toehold itself.  The inverse, for the
// chain walks, is rbg_chain_walk.hpp chain_toehold: the two change together.
__device__ __forceinline__ uint64_t locus_key(const DevIndex &ix, const uint64_t k) {
    if (k >= ix.n) return ~uint64_t(0);
    uint32_t a = 0, z = ix.order_ndocs;          // the last document that starts at or before k (doclist.hpp:46-50: a predecessor query)
    while (z - a > 1u) {
        const uint32_t m = (a + z) >> 1;
        if (ix.order_docs[m] <= k) a = m; else z = m;
    }
    const uint64_t o = k - ix.order_docs[a];
    const uint32_t low = ix.order_lowbits, db = ix.order_dbits;
    return ((o >> low) << (db + low)) | (static_cast<uint64_t>(a) << low) | (o & ((uint64_t(1) << low) - 1u));
}
// 4-byte positions, absolute order: the sort moves 32-bit keys (a third fewer bytes per radix pass than 64-bit ones).  A toehold outside the text
// (it wrapped below zero) travels as 0xFFFFFFFF -- no position of an index with 4-byte positions -- and K3 reads the toehold itself.
__global__ __launch_bounds__(256) void k_keys32(const DevIndex ix, const uint64_t *__restrict__ k, const uint64_t N, uint32_t *__restrict__ keys, uint32_t *__restrict__ iota) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < N; i += stride) {
        const uint64_t v = k[i];
        keys[i] = v >= ix.n ? 0xFFFFFFFFu : static_cast<uint32_t>(v);
        iota[i] = static_cast<uint32_t>(i);
    }
}
__global__ __launch_bounds__(256) void k_locus_keys(const DevIndex ix, const uint64_t *__restrict__ k, const uint64_t N, uint64_t *__restrict__ keys,
                                                    uint32_t *__restrict__ iota) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < N; i += stride) {
        keys[i] = locus_key(ix, k[i]);
        iota[i] = static_cast<uint32_t>(i);
    }
}

template <typename P>
__device__ __forceinline__ uint64_t phi_step(const DevIndex &ix, uint64_t i, bool *searched = nullptr) {
    const PhiSlot<P> *__restrict__ slots = static_cast<const PhiSlot<P> *>(ix.phi_slots);
    if (i >= ix.n) {
        // Only a toehold that wrapped below zero gets here: a match at text position 0 leaves k - 1 =
        // 2^64 - 1 (LF_w_loc, rowbowt.hpp:561).  The reference's phi is outside its domain there
        // (toehold_sa.hpp:57-59 assert); its arithmetic on the last sampled position is followed, and no
        // table is indexed with the out-of-range value.
        const PhiEnt<P> e = static_cast<const PhiEnt<P> *>(ix.phi_ent)[ix.r - 1];
        const uint64_t sum = static_cast<uint64_t>(e.base) + (i - static_cast<uint64_t>(e.pos));  // wraps like uint64_t there
        return sum % ix.n;
    }
    const uint64_t b = i >> ix.phi_shift;
    // the slot as {dprev, d0, d1, off0, off1, cnt}: 4 x P, or the 16-byte packed form at 8-byte positions (rbg_dev.h)
    uint64_t dprev, d0, d1;
    uint32_t off0, off1, cnt;
    if (sizeof(P) == 8 && ix.phi_packed) {
        const uint4 raw = load_slot(static_cast<const uint4 *>(ix.phi_slots) + b);
        const uint64_t w0 = static_cast<uint64_t>(raw.x) | (static_cast<uint64_t>(raw.y) << 32);
        const uint64_t w1 = static_cast<uint64_t>(raw.z) | (static_cast<uint64_t>(raw.w) << 32);
        constexpr uint64_t M38 = (uint64_t(1) << 38) - 1;
        dprev = w0 & M38;
        d0 = (w0 >> 38) | ((w1 & 0xFFFull) << 26);
        d1 = (w1 >> 12) & M38;
        cnt = static_cast<uint32_t>(w1 >> 62);
        off0 = cnt >= 1 ? static_cast<uint32_t>(w1 >> 50) & 63u : 0xFFu;   // (absent offsets compare as "never above")
        off1 = cnt == 2 ? static_cast<uint32_t>(w1 >> 56) & 63u : 0xFFu;
    } else {
        const PhiSlot<P> sl = load_slot(slots + b);
        const uint32_t meta = static_cast<uint32_t>(sl.meta);
        dprev = sl.dprev; d0 = sl.d0; d1 = sl.d1;
        off0 = meta & 0xFFu; off1 = (meta >> 8) & 0xFFu; cnt = (meta >> 16) & 3u;
    }
    uint64_t s;
    if (cnt == kPhiOvf) {
        if (searched) *searched = true;
        const PhiEnt<P> *__restrict__ ent = static_cast<const PhiEnt<P> *>(ix.phi_ent);
        uint64_t a = ix.phi_ord[b], z = ix.phi_ord[b + 1];
        while (z - a > 4) {
            const uint64_t mid = a + ((z - a) >> 1);
            if (static_cast<uint64_t>(ent[mid].pos) < i) a = mid + 1; else z = mid;
        }
        while (a < z && static_cast<uint64_t>(ent[a].pos) < i) ++a;
        // a == pred_.rank(i); circular predecessor (sparse_sd_vector.hpp:141-143)
        const PhiEnt<P> e = ent[a ? a - 1 : ix.r - 1];
        const uint64_t j = e.pos;
        const uint64_t delta = j < i ? i - j : i + 1;  // toehold_sa.hpp:65
        s = static_cast<uint64_t>(e.base) + delta;
    } else {
        const uint32_t o = static_cast<uint32_t>(i - (b << ix.phi_shift));
        uint64_t D = dprev;
        if (o > off0) D = d0;
        if (o > off1) D = d1;
        s = D + i;  // D = (base - pos) mod n of the predecessor: base + (i - pos)
    }
    if (s >= ix.n) s -= ix.n;  // (prev_sample + delta) % n_ (toehold_sa.hpp:71); s < 2n
    return s;
}

// phi_step as the chain walks take it (rbg_chain_walk.hpp, rbg_locate_docs.hpp): under STATS a searched step (an overflowing slot) adds 1 to `cost`
template <typename P, bool STATS = false>
__device__ __forceinline__ uint64_t slot_phi(const DevIndex &ix, const uint64_t k1, unsigned long long &cost) {
    if (!STATS) return phi_step<P>(ix, k1);
    bool searched = false;
    const uint64_t s = phi_step<P>(ix, k1, &searched);
    cost += searched ? 1 : 0;
    return s;
}

// K3 over the phi slots: rbg_chain_walk.hpp chain_fill_walk (the walk, its staging and what the template parameters mean) with phi_step as its phi.
// Flush windows of eight locations = 64 bytes at both position widths (the measurements: rbg_chain_walk.hpp).
#ifndef RBG_K3_CHUNK_U32
#define RBG_K3_CHUNK_U32 8
#endif
constexpr int kChunk = RBG_K3_CHUNK_U32;
#ifndef RBG_K3_CHUNK_U64
#define RBG_K3_CHUNK_U64 8
#endif

template <typename P, bool STATS = false, typename OUT = uint64_t, bool SUB = false, bool HI8 = false, int CH = (sizeof(P) == 8 ? RBG_K3_CHUNK_U64 : kChunk), bool RING = true>
__global__ __launch_bounds__(256, (chain_stage_waves<ChainStage<P, CH, SUB, RING, HI8>>())) void k_locate_fill(const DevIndex ix, const uint64_t *__restrict__ lo,
                                                        const uint64_t *__restrict__ hi, const uint64_t *__restrict__ k,
                                                        const uint64_t N, const uint64_t max_hits,
                                                        const uint64_t *__restrict__ loc_off, OUT *__restrict__ locs,
                                                        const uint64_t *__restrict__ sub, const uint32_t *__restrict__ order,
                                                        const uint64_t *__restrict__ skeys,
                                                        unsigned long long *__restrict__ stats = nullptr) {
    using Stage = ChainStage<P, CH, SUB, RING, HI8>;
    __shared__ Stage S;
    chain_fill_walk<P, OUT, STATS, SUB, HI8, CH, CH>(ix, S, lo, hi, k, N, max_hits, loc_off, locs, sub, order, skeys, stats,
                                                     [&](const uint64_t k1, unsigned long long &cost) { return slot_phi<P, STATS>(ix, k1, cost); });
}

// ---- document hits from the walk itself (rbg_locate_docs.hpp): k_locate_fill's chains, the positions resolved and reduced instead of stored ----
// LAUNCH BOUNDS: 256 threads; tools/kernel_resources.py lists registers and scratch (none).  The dynamic LDS is what the table needs.
extern __shared__ unsigned long long locate_docs_lds[];
template <typename P, bool LOCS>
__global__ __launch_bounds__(kLocDocBlock) void k_locate_docs(const DevIndex ix, const DocTable t, const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi,
                                                             const uint64_t *__restrict__ k, const uint64_t N, const uint64_t max_hits,
                                                             const uint32_t *__restrict__ order, const uint64_t *__restrict__ skeys, uint64_t *__restrict__ sets,
                                                             uint32_t *__restrict__ ndocs_out, uint32_t *__restrict__ nodoc_out,
                                                             unsigned long long *__restrict__ doc_reads, unsigned long long *__restrict__ doc_locs) {
    locate_docs_walk<P, LOCS>(ix, t, locate_docs_lds, lo, hi, k, N, max_hits, order, skeys, sets, ndocs_out, nodoc_out, doc_reads, doc_locs,
                              [&](const uint64_t k1, unsigned long long &cost) { return slot_phi<P>(ix, k1, cost); });
}

}  // namespace

// ---- chain ordering for locate: permutation of the reads by toehold value (radix sort) ----------
namespace {
__global__ __launch_bounds__(256) void k_iota(uint32_t *__restrict__ v, const uint64_t N) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < N; i += stride) v[i] = static_cast<uint32_t>(i);
}
struct OrderWs {
    size_t perm, iota, keys, keys_in, sort, sort_bytes, total;   // keys_in: the locus keys the sort reads (the absolute order sorts the toeholds where they are)
};
OrderWs order_layout(uint64_t N) {
    auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
    OrderWs w{};
    w.perm = 0;
    w.iota = up(w.perm + N * 4);
    w.keys = up(w.iota + N * 4);
    w.keys_in = up(w.keys + N * 8);
    w.sort = up(w.keys_in + N * 8);
    size_t bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, static_cast<const uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr),
                                             static_cast<const uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr),
                                             static_cast<int64_t>(N ? N : 1), 0, 64);
    w.sort_bytes = bytes;
    w.total = up(w.sort + bytes) + 256;
    return w;
}
}  // namespace

size_t locate_order_ws_bytes(uint64_t N) { return order_layout(N).total; }

int launch_locate_order(const DevIndex &ix, const LaunchCfg &cfg, const uint64_t *k, uint64_t N, void *ws, size_t ws_bytes,
                        void *stream) {
    if (N == 0) return 0;
    if (N >= 0xFFFFFFFFull) return static_cast<int>(hipErrorInvalidValue);  // permutation entries are 32-bit
    const OrderWs w = order_layout(N);
    if (ws_bytes < w.total || (reinterpret_cast<uintptr_t>(ws) & 255)) return static_cast<int>(hipErrorInvalidValue);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *base = static_cast<char *>(ws);
    uint32_t *perm = reinterpret_cast<uint32_t *>(base + w.perm);
    uint32_t *iota = reinterpret_cast<uint32_t *>(base + w.iota);
    uint64_t *keys = reinterpret_cast<uint64_t *>(base + w.keys);
    if (ix.order_docs) {   // locus order: sort the keys {offset >> low, document, ...} on the bits above `low`
        uint64_t *keys_in = reinterpret_cast<uint64_t *>(base + w.keys_in);
        hipLaunchKernelGGL(k_locus_keys, dim3(grid_for(cfg, N)), dim3(256), 0, st, ix, k, N, keys_in, iota);
        int rc0 = static_cast<int>(hipGetLastError());
        if (rc0) return rc0;
        size_t bytes0 = w.sort_bytes;
        // (all 64 bits when a toehold may have wrapped: its all-ones key sorts last either way; the bits above obits + dbits are zero otherwise)
        const int lo_bit = static_cast<int>(ix.order_lowbits), hi_bit = static_cast<int>(ix.order_obits + ix.order_dbits) + 1;
        return static_cast<int>(hipcub::DeviceRadixSort::SortPairs(base + w.sort, bytes0, keys_in, keys, iota, perm, static_cast<int64_t>(N), lo_bit, hi_bit < 64 ? hi_bit : 64, st));
    }
    int end_bit = 1;
    while (end_bit < 64 && (ix.n >> end_bit)) ++end_bit;  // toeholds are text positions < n
    if (ix.pos_bytes == 4) {   // 32-bit keys (k_keys32): the key pass also makes the identity permutation
        uint32_t *k32_in = reinterpret_cast<uint32_t *>(base + w.keys_in), *k32_out = reinterpret_cast<uint32_t *>(base + w.keys);
        // (computing the keys where the sort reads them -- rocprim iterators, no key pass -- reads the 8-byte toeholds twice: 0.331 -> 0.337 ms, profiles/r06_experiments.txt)
        hipLaunchKernelGGL(k_keys32, dim3(grid_for(cfg, N)), dim3(256), 0, st, ix, k, N, k32_in, iota);
        int rc32 = static_cast<int>(hipGetLastError());
        if (rc32) return rc32;
        int b0 = static_cast<int>(ix.phi_shift) + 2;
        if (end_bit - b0 < 8) b0 = 0;
        size_t bytes32 = w.sort_bytes;   // (sized for 64-bit keys: enough for 32-bit ones)
        return static_cast<int>(hipcub::DeviceRadixSort::SortPairs(base + w.sort, bytes32, k32_in, k32_out, iota, perm, static_cast<int64_t>(N), b0, end_bit < 32 ? end_bit : 32, st));
    }
    hipLaunchKernelGGL(k_iota, dim3(grid_for(cfg, N)), dim3(256), 0, st, iota, N);
    int rc = static_cast<int>(hipGetLastError());
    if (rc) return rc;
    // the order only has to bring chains of nearby text positions together: the low bits (positions
    // inside one 64-byte line of phi slots) need no sorting, which saves a radix pass
    int begin_bit = static_cast<int>(ix.phi_shift) + 2;
    if (end_bit - begin_bit < 8) begin_bit = 0;
    // (sorting on fewer, higher bits costs K3 what it saves the sort: profiles/r06_experiments.txt)
    size_t bytes = w.sort_bytes;
    return static_cast<int>(hipcub::DeviceRadixSort::SortPairs(base + w.sort, bytes, k, keys, iota, perm, static_cast<int64_t>(N),
                                                               begin_bit, end_bit, st));
}

size_t scan_tmp_bytes(uint64_t N) {
    size_t bytes = 0;
    uint64_t *p = nullptr;
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, bytes, p, p, static_cast<int64_t>(N ? N : 1));
    return bytes + 256;
}

// occ(i) = min(hi - lo + 1, max_hits) or 0 (toehold_sa.hpp:38-39), computed where the scan reads it: the plan is ONE pass over (lo, hi) -- until
// round 6 a kernel wrote the counts and the scan read them back (0.126 -> 0.09 ms per 10 M reads)
struct OccOf {
    const uint64_t *lo, *hi;
    uint64_t max_hits;
    __host__ __device__ __forceinline__ uint64_t operator()(const uint64_t i) const {
        const uint64_t l = lo[i], h = hi[i];
        uint64_t occ = h >= l ? h - l + 1 : 0;
        return occ > max_hits ? max_hits : occ;
    }
};
__global__ void k_zero_u64(uint64_t *p) { *p = 0; }

int launch_locate_plan(const DevIndex &ix, const LaunchCfg &cfg, const uint64_t *lo, const uint64_t *hi, uint64_t N,
                       uint64_t max_hits, uint64_t *loc_off, void *tmp, size_t tmp_bytes, void *stream) {
    (void)ix; (void)cfg;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_zero_u64, dim3(1), dim3(1), 0, st, loc_off);
    int rc = static_cast<int>(hipGetLastError());
    if (rc || N == 0) return rc;
    hipcub::TransformInputIterator<uint64_t, OccOf, hipcub::CountingInputIterator<uint64_t>> in(hipcub::CountingInputIterator<uint64_t>(0), OccOf{lo, hi, max_hits});
    size_t need = 0;
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, need, in, loc_off + 1, static_cast<int64_t>(N));
    tmp = scan_scratch(tmp, tmp_bytes);
    if (need > tmp_bytes) return static_cast<int>(hipErrorInvalidValue);
    return static_cast<int>(hipcub::DeviceScan::InclusiveSum(tmp, need, in, loc_off + 1, static_cast<int64_t>(N), st));
}

int launch_locate_fill(const DevIndex &ix, const LaunchCfg &cfg, const uint64_t *lo, const uint64_t *hi,
                       const uint64_t *k, uint64_t N, uint64_t max_hits, const uint64_t *loc_off, uint64_t *locs,
                       const uint64_t *sub, const void *order, void *stream, unsigned long long *stats, uint32_t *locs32) {
    if (N == 0) return 0;
    // (the grid: up to 32 workgroups per CU looping over the chains; 8 / 16 / 64 per CU and one workgroup per 256 chains without a loop measured
    //  level or worse within the processes' spread: profiles/r06_experiments.txt)
    const dim3 grid(grid_for(cfg, N)), block(cfg.block_threads);
    // the order workspace also holds the toeholds in sorted order (launch_locate_order's key output)
    const uint64_t *skeys = order ? reinterpret_cast<const uint64_t *>(static_cast<const char *>(order) + order_layout(N).keys) : nullptr;
    const uint32_t *perm = static_cast<const uint32_t *>(order);
    if (ix.layout == 2 && !ix.phi_slots) {  // run-indexed layout (k_runs.hip); with phi slots (RBG_OPT_RUN_PHI) the slot kernels below answer its phi
        return launch_locate_fill_runs(ix, cfg, lo, hi, k, N, max_hits, loc_off, locs, sub, order, skeys, stream, stats, locs32);
    }
    return chain_fill_variants(ix, stats, sub, locs, locs32, [&](auto p, auto sts, auto sb, auto h8, auto *dst) {
        return launch_grid(k_locate_fill<pos_t<decltype(p)>, decltype(sts)::value, std::remove_pointer_t<decltype(dst)>, decltype(sb)::value, decltype(h8)::value>,
                           grid, block, 0, stream, ix, lo, hi, k, N, max_hits, loc_off, dst, sub, perm, skeys, stats);
    });
}

int launch_locate_doc_hits(const DevIndex &ix, const LaunchCfg &cfg, const DocTable &t, const uint64_t *lo, const uint64_t *hi, const uint64_t *k, uint64_t N,
                           uint64_t max_hits, const void *order, uint64_t *sets, uint32_t *ndocs_out, uint32_t *nodoc_out, uint64_t *doc_reads,
                           uint64_t *doc_locs, void *stream) {
    (void)cfg;
    if (t.ndocs == 0 || t.ndocs > kLocDocLdsDocs) return static_cast<int>(hipErrorInvalidValue);
    if (N == 0) return 0;
    if (order && N >= 0xFFFFFFFFull) return static_cast<int>(hipErrorInvalidValue);   // (launch_locate_order refuses it too)
    const uint64_t *skeys = order ? reinterpret_cast<const uint64_t *>(static_cast<const char *>(order) + order_layout(N).keys) : nullptr;
    if (ix.layout == 2 && !ix.phi_slots)   // run-indexed layout with the phi list (k_runs.hip); with phi slots the kernels here answer its phi
        return launch_locate_doc_hits_runs(ix, t, lo, hi, k, N, max_hits, order, skeys, sets, ndocs_out, nodoc_out, doc_reads, doc_locs, stream);
    const dim3 grid(locate_docs_grid(N)), block(kLocDocBlock);
    const uint32_t *perm = static_cast<const uint32_t *>(order);
    unsigned long long *dr = reinterpret_cast<unsigned long long *>(doc_reads), *dl = reinterpret_cast<unsigned long long *>(doc_locs);
    const size_t lds = locate_docs_lds_bytes(t.ndocs, t.ndir, doc_locs != nullptr);
    return with_pos(ix.pos_bytes, [&](auto p) { return with_flag(doc_locs != nullptr, [&](auto lc) {
        return launch_lds(k_locate_docs<pos_t<decltype(p)>, decltype(lc)::value>, grid, block, lds, 0, stream,
                          ix, t, lo, hi, k, N, max_hits, perm, skeys, sets, ndocs_out, nodoc_out, dr, dl);
    }); });
}

}  // namespace rbg
