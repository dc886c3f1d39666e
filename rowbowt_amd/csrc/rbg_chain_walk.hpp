// rbg_chain_walk.hpp -- K3's chain walk (ToeholdSA::locate_range, toehold_sa.hpp:37-49), written once for both layouts: the decode of a read's toehold from
// the order workspace, the body of the fill kernels (k_locate.hip k_locate_fill, k_runs.hip k_locate_fill_runs2) and the list of their variants.  What differs
// between the layouts is how `k <- phi(k)` is answered, and that comes in as `phi` (k_locate.hip slot_phi, rbg_runs2_device.hpp run_phi) -- as it does in the
// document-hits walk (rbg_locate_docs.hpp), which shares the decode and the phi steps but not the loop.
#pragma once

#include "rbg_device.hpp"
#include "rbg_dispatch.hpp"

namespace rbg {
namespace {

// The toehold of read i = order[j] from the sorted keys of launch_locate_order (k_locate.hip), by the key that order used:
//   the locus key (ix.order_docs; the inverse of k_locate.hip locus_key): {offset >> low, document, offset & (2^low - 1)} -> order_docs[document] + offset;
//   the 32-bit key of 4-byte positions (k_locate.hip k_keys32): the toehold itself;
//   the plain 64-bit toehold.
// A toehold outside the text (it wrapped below zero) has no document and is no 32-bit position: it travels as the all-ones key and is read from k[i].  So k
// must still hold what the order was computed from, and the document table must be the one of that call (include/rbg.h rbg_locate_order_dev).
template <typename P>
__device__ __forceinline__ uint64_t chain_toehold(const DevIndex &ix, const uint64_t *__restrict__ skeys, const uint64_t *__restrict__ k, const uint64_t i,
                                                  const uint64_t j) {
    if (ix.order_docs) {
        const uint64_t key = skeys[j];
        if (key == ~uint64_t(0)) return k[i];
        const uint32_t low = ix.order_lowbits, db = ix.order_dbits;
        const uint64_t doc = (key >> low) & ((uint64_t(1) << db) - 1u);
        return ix.order_docs[doc] + (((key >> (db + low)) << low) | (key & ((uint64_t(1) << low) - 1u)));
    }
    if (sizeof(P) == 4) {
        const uint32_t k32 = reinterpret_cast<const uint32_t *>(skeys)[j];
        return k32 == 0xFFFFFFFFu ? k[i] : k32;
    }
    return skeys[j];
}

// The body of both fill kernels.  One lane walks one read's phi chain; the chain is serial, the reads are not.  The values are staged per wave in LDS, CH steps
// at a time, and flushed as WINDOWS of CH locations on boundaries of the output array, CH lanes per read (rbg_device.hpp ChainStage: what is staged, why, and
// what it costs in LDS).  Eight steps = 64-byte windows at both position widths since the windows are aligned (profiles/r06_k3_ring_ab.txt); with unaligned
// segments sixteen steps were better at 4-byte positions (3.5 / 3.1 / 3.5 ms per 10 M reads at 8 / 16 / 32, round 3) -- a 64-byte store on a 64-byte boundary
// runs at 2.9 TB/s, a 128-byte one wherever it falls at 1.2.
// (Line-aligned flush segments -- a lane waiting `dst mod CH` columns before its first step so that every flush writes whole lines -- lost twice and were
//  retired with the round-3 staging: on the bench index in round 3, and at r = 1.2e8 in round 6 (11.1 -> 14.9 ms, profiles/r06_k3_align_ab.txt): lanes that wait
//  a different number of columns fall out of PHASE, and chains of one locus walking in phase -- neighbouring lanes asking for the same phi sector in the same
//  instruction -- is what K3's speed rests on.)
// phi(k1, cost) = the position before k1 in the chain; under STATS it adds its layout's price of the step to `cost`, which leaves as stats[kLsPhiOvf].
// STATS = the instrumented instantiation (rbg_locate_fill_stats_dev): the same walk plus the LocateStat sums.
// OUT = the width a location is stored at: uint64_t (the API's, toehold_sa.hpp:37-49 fills a vector<uint64_t>) or, for device pipelines on an index with
// 4-byte positions, uint32_t (rbg_locate_fill_dev32: half the write requests; the low 32 bits of the same values, so a toehold that wrapped below zero reads
// 0xFFFFFFFF).
// SUB = `sub` is subtracted from every location (locate_from_longest_seed, rowbowt.hpp:681-683).
// UNROLL = the unroll count of the loop over a round's steps (CH: all of them).
template <typename P, typename OUT, bool STATS, bool SUB, bool HI8, int CH, int UNROLL, bool RING, typename Phi>
__device__ __forceinline__ void chain_fill_walk(const DevIndex &ix, ChainStage<P, CH, SUB, RING, HI8> &S, const uint64_t *__restrict__ lo,
                                                const uint64_t *__restrict__ hi, const uint64_t *__restrict__ k, const uint64_t N, const uint64_t max_hits,
                                                const uint64_t *__restrict__ loc_off, OUT *__restrict__ locs, const uint64_t *__restrict__ sub,
                                                const uint32_t *__restrict__ order, const uint64_t *__restrict__ skeys, unsigned long long *__restrict__ stats,
                                                Phi phi) {
    using Stage = ChainStage<P, CH, SUB, RING, HI8>;
    const uint64_t out_elem0 = reinterpret_cast<uintptr_t>(locs) / sizeof(OUT);
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    unsigned long long c_locs = 0;
    unsigned long long st_phi = 0, st_cost = 0, st_chains = 0;  // STATS only
    const uint32_t block = __builtin_amdgcn_workgroup_size_x();   // (blockDim.x read in a device function stays a per-lane value: the stride in two VGPRs)
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * block;
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * block + wv * kWave; base < N; base += stride) {
        // `order` (optional) lists the reads by toehold text position: neighbouring lanes then walk
        // neighbouring phi slots (same DRAM rows / L2 lines) for the whole chain, because the chains of
        // reads from nearby loci visit the haplotypes in the same order.  Results land at loc_off[i]
        // whatever the processing order.
        const uint64_t j = base + lane;
        uint64_t i = j;
        if (order && j < N) i = order[j];
        uint64_t occ = 0, k1 = 0, dst = 0;
        if (i < N) {
            dst = loc_off[i];
            if (skeys) {
                // ordered walk: the toehold travels with the sort (sequential read) and the count is the
                // planned one, loc_off[i+1] - loc_off[i] = min(occ, max_hits): one random 64-byte sector
                // per read instead of four (lo, hi, k, loc_off)
                k1 = chain_toehold<P>(ix, skeys, k, i, j);
                occ = loc_off[i + 1] - dst;
            } else {
                const uint64_t l = lo[i], h = hi[i];
                occ = h >= l ? h - l + 1 : 0;  // toehold_sa.hpp:38-39
                if (occ > max_hits) occ = max_hits;
                k1 = k[i];
            }
        }
        const uint64_t minus = (SUB && i < N) ? sub[i] : 0;
        // the window grid of this read: its first location sits a elements past a CH-element boundary of the output array (RING; else a = 0)
        const uint32_t a = (RING && occ) ? static_cast<uint32_t>((out_elem0 + dst) & static_cast<uint64_t>(CH - 1)) : 0u;
        S.dst[wv][lane] = dst - a;   // (wraps for a read at the very start of a misaligned array; + v >= a brings it back)
        if (SUB) S.minus[wv][lane] = minus;
        // the toehold itself is not a text position when it wrapped (2^64 - 1): at 4-byte positions its owner stores that location (ChainStage)
        const bool off_text = Stage::kSentinel && k1 >= ix.n;
        if (off_text && occ) locs[dst] = static_cast<OUT>(k1 - minus);
        c_locs += occ;
        if (STATS && occ) st_chains += 1;
        uint64_t wmax = occ + a;      // the chain's extent in virtual columns
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            const uint64_t other = __shfl_xor(wmax, o, kWave);
            wmax = other > wmax ? other : wmax;
        }
        for (uint64_t t0 = 0; t0 < wmax; t0 += CH) {
            const uint32_t cnt = chain_round_count<CH>(occ, t0);
            S.bounds[wv][lane] = chain_window_bounds<CH>(occ, a, t0);
#pragma unroll UNROLL
            for (int e = 0; e < CH; ++e) {
                const bool mine = static_cast<uint32_t>(e) < cnt;
                if (mine && (e || t0)) {   // every location but a read's first is phi of the one before (toehold_sa.hpp:44)
                    k1 = phi(k1, st_cost);
                    if (STATS) st_phi += 1;
                }
                if (mine) chain_put(S, wv, lane, a + static_cast<uint32_t>(t0) + e, k1, e == 0 && t0 == 0 && off_text);
            }
            wave_lds_sync();
            chain_flush(S, wv, lane, t0, locs);
            wave_lds_sync();
        }
        wave_lds_sync();
    }
    c_locs = wave_sum(c_locs);
    if (lane == 0 && c_locs) atomicAdd(&ix.counters[3], c_locs);
    if (STATS) {
        st_phi = wave_sum(st_phi);
        st_cost = wave_sum(st_cost);
        st_chains = wave_sum(st_chains);
        if (lane == 0) {
            if (st_phi) atomicAdd(&stats[kLsPhiSteps], st_phi);
            if (st_cost) atomicAdd(&stats[kLsPhiOvf], st_cost);
            if (st_chains) atomicAdd(&stats[kLsChains], st_chains);
            if (c_locs) atomicAdd(&stats[kLsLocs], c_locs);
        }
    }
}

}  // namespace

// The fill kernels' variants that exist, and the calls that are refused, for launch_locate_fill (k_locate.hip) and launch_locate_fill_runs (k_runs.hip):
// 4-byte locations at 4-byte positions, instrumented, sub-ranges, plain, each with HI8 (rbg_device.hpp ChainStage: a value as its low word + one high byte;
// RBG_K3_HI8=0 -- tests -- stages whole 8-byte values at any n) at 8-byte positions only.  launch(p, sts, sb, h8, dst) names the kernel (rbg_dispatch.hpp: the
// rule about subsets): P = pos_t<decltype(p)>, STATS, SUB and HI8 the values of the tags, OUT what dst points to.
template <typename F>
int chain_fill_variants(const DevIndex &ix, unsigned long long *stats, const uint64_t *sub, uint64_t *locs, uint32_t *locs32, F &&launch) {
    if ((stats || locs32) && sub) return static_cast<int>(hipErrorInvalidValue);
    if (locs32 && ix.pos_bytes != 4) return static_cast<int>(hipErrorInvalidValue);   // 4-byte locations: 4-byte positions only (the caller checked)
    const bool hi8 = ix.pos_bytes == 8 && ix.n < kChainHi8Limit && chain_hi8_enabled();
    return with_pos(ix.pos_bytes, [&](auto p) {
        auto fill = [&](auto sts, auto sb, auto *dst) {
            return with_flag(hi8, [&](auto h8) { return launch(p, sts, sb, std::bool_constant<sizeof(pos_t<decltype(p)>) == 8 && decltype(h8)::value>{}, dst); });
        };
        if constexpr (sizeof(pos_t<decltype(p)>) == 4) { if (locs32) return fill(no, no, locs32); }
        if (stats) return fill(yes, no, locs);
        if (sub) return fill(no, yes, locs);
        return fill(no, no, locs);
    });
}

}  // namespace rbg
