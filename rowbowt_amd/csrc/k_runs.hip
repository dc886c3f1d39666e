// k_runs.hip -- the run-indexed layout (RBG_LAYOUT_RUNS): K1/K2 and K3 with space proportional to r.  rank and phi are
// predecessor searches over sorted run boundaries, as in the reference (rle_string::rank rle_string.hpp:131-161,
// ToeholdSA::phi toehold_sa.hpp:56-72): a directory (or a bucket record) has already cut the search down to the handful
// of entries of one bucket, and the lane that owns the query fetches and scans exactly those (rbg_runs2_device.hpp).  One
// lane owns one read (K1/K2) or one phi chain (K3); bucket records are fetched by quads of lanes.
#include <type_traits>

#include "rbg_runs2_device.hpp"
#include "rbg_chain_walk.hpp"
#include "rbg_locate_docs.hpp"
#include "rbg_jump.h"
#include "rbg_launch.hpp"

namespace rbg {
namespace {

// ---- K1 / K2 over the run-indexed layout ------------------------------------------------------------------------
// RowBowt::find_range (rowbowt.hpp:121-131) / find_range_w_toehold (:169-184).  A step consumes up to run_ksteps read
// symbols through the k-mer depth's table, exactly as k_find_range does with its slot tables (k_search.hip; DESIGN.md
// 2b: identical to that many nested RowBowt::LF / LF_w_loc calls, rowbowt.hpp:74-88, :555-573); both ranks of all
// the wave's reads are answered cooperatively.  The device ftab (a constant-size state table, result-neutral) still
// replaces the first ftab_k steps.
// (4 waves per SIMD at 4-byte positions: the toehold variant sits at 130 VGPRs without the bound, one wave per SIMD less)
// PACKED: the reads arrive as 2-bit codes (k_pack_reads / the host path's CPU packer: meta[i] = {first chunk, length or
// bit 31 = "has a symbol outside the k-mer alphabet: byte kernel"}, 64 symbols per 16-byte chunk in consumption order);
// same steps in the same order as the byte form takes for a read of k-mer symbols only.
// STATS: the instrumented instantiation (rbg_find_range_stats_dev), sums as listed in rbg_runs_device.hpp.
struct PackedBits {   // per-lane reader of a packed read: peek / drop of up to 32 bits
    const uint4 *__restrict__ cp;
    uint4 w;
    uint32_t widx, navail;
    uint64_t sr;
    __device__ __forceinline__ uint32_t next_word() {
        if (widx == 4) { w = *cp++; widx = 0; }
        // (the word in front, the others moved up: indexing the vector by widx becomes a dynamic index, and one into scratch once the
        //  reader is captured by the step's lambda)
        const uint32_t v = w.x;
        w.x = w.y; w.y = w.z; w.z = w.w;
        ++widx;
        return v;
    }
    __device__ __forceinline__ uint32_t take(uint32_t nb) {
        if (navail < nb) { sr |= static_cast<uint64_t>(next_word()) << navail; navail += 32; }
        const uint32_t v = static_cast<uint32_t>(sr & ((uint64_t(1) << nb) - 1));
        sr >>= nb;
        navail -= nb;
        return v;
    }
};

// The probe of the jump table (rbg_jump.h) by the whole wave: EVERY lane calls, `probing` says whether the lane has a key to look up.  A lane
// reading its own 64-byte bucket would issue two to four 16-byte requests to one sector, in up to three dependent round trips (slot 0, slot 1,
// the next bucket); here the lane's quad fetches the bucket as one request (rbg_runs2_device.hpp quad_fetch_issue / _take, as the bucket records
// of the steps) and jump_bucket settles both slots from its sixteen words.  A lane that is not probing, or has its answer, names bucket 0 of
// the table; the rounds go on while any lane's chain does (about 0.2 buckets per read beyond the first).  `tile` (GLDS) must be free: no step
// is in flight.  Returns true on a hit (v = {lo, hi, toehold}); buckets = buckets this lane's probe read.
template <bool GLDS>
__device__ __forceinline__ bool jump_probe_wave(const void *__restrict__ tab, const uint64_t nb, const bool probing, const JumpKey &key, uint32_t v[3],
                                                uint32_t &buckets, lds_byte *tile) {
    uint32_t state = probing ? kJumpNext : kJumpAbsent;           // kJumpNext: undecided, the bucket `b` is the next to read
    uint64_t b = probing ? jump_home(jump_hash(key), nb) : 0u;
    uint64_t left = nb;                                            // at most nb buckets (jump_probe)
    while (__ballot(state == kJumpNext)) {
        const bool undecided = state == kJumpNext;
        uint32_t w[16];
        quad_fetch_issue<GLDS>(reinterpret_cast<uint64_t>(tab) + (undecided ? b : 0u) * kJumpBucketBytes, w, tile);
        quad_fetch_take<GLDS>(w, tile);
        if (undecided) {
            ++buckets;
            state = jump_bucket(w, key, v);
            b = jump_next(b, nb);
            if (--left == 0 && state == kJumpNext) state = kJumpAbsent;
        }
    }
    return state <= kJumpHit1;
}

// a 64-bit value every lane holds alike (read from LDS), as scalars
__device__ __forceinline__ uint64_t uniform_u64(const uint64_t v) {
    // (the builtin returns int: through uint32_t, or the low half is sign-extended over the high one)
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v)));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32)));
    return static_cast<uint64_t>(lo) | (static_cast<uint64_t>(hi) << 32);
}

// word j of a lane's staged read (rbg_runs_device.hpp: the lane's column, word w at codes[64 w]), for jump_key_from_codes
struct StagedWords {
    const lds_u32 *codes;
    __device__ __forceinline__ uint32_t operator()(const uint32_t j) const { return codes[64u * j]; }
};

// (the staging of a wave's reads as 2-bit codes in LDS -- stage_read, StageTab, kStageCap -- lives in rbg_runs_device.hpp: the seeding kernels use it too)
// GLDS: the bucket records arrive by LDS-direct loads (rbg_runs2_device.hpp lane_lf2_quad) instead of quad permutes
// STAGE (byte form only): the wave stages its reads as 2-bit codes in LDS first (above)
template <typename P, bool TOEHOLD, bool PACKED = false, bool STATS = false, bool GLDS = false, bool STAGE = false>
__global__ __launch_bounds__(512, STATS ? 2 : 4) void k_find_range_runs(const DevIndex ix, const void *__restrict__ src_a,
                                                        const void *__restrict__ src_b, const uint64_t N,
                                                        uint64_t *__restrict__ lo_out, uint64_t *__restrict__ hi_out,
                                                        uint64_t *__restrict__ ss_out, unsigned long long *__restrict__ stats,
                                                        const uint32_t *__restrict__ sel, const uint32_t *__restrict__ nsel) {
    // byte form: src_a = seqs, src_b = off;  packed form: src_a = chunks (uint4), src_b = meta (uint2)
    // sel != nullptr (byte form): only the reads sel[0 .. *nsel) -- the ones the packed form could not express
    const uint64_t Neff = sel ? static_cast<uint64_t>(*nsel) : N;
    const uint8_t *__restrict__ seqs = static_cast<const uint8_t *>(src_a);
    const uint64_t *__restrict__ off = static_cast<const uint64_t *>(src_b);
    const uint4 *__restrict__ chunks = static_cast<const uint4 *>(src_a);
    const uint2 *__restrict__ meta = static_cast<const uint2 *>(src_b);
    __shared__ uint8_t s_lut[256];
    __shared__ uint8_t s_lut2[256];
    __shared__ uint8_t s_mslot[4];
    __shared__ __align__(16) unsigned char s_tile[GLDS ? 8 * kTileBytes : 16];   // (eight waves per workgroup)
    __shared__ uint32_t s_codes[STAGE ? 8 * kStageWords * 64 : 1];               // STAGE: the waves' reads as 2-bit codes
    // the jump table's levels {table, buckets, K} (STAGE): the probe loop reads its level's from here -- both levels' held in scalar
    // registers across the loop were nine more than the kernel has
    __shared__ uint64_t s_jump[STAGE ? 4 : 1];
    __shared__ uint32_t s_jump_k[STAGE ? 2 : 1];
    for (int t = threadIdx.x; t < 256; t += blockDim.x) {
        s_lut[t] = ix.lut[t];
        s_lut2[t] = ix.nmajor ? ix.lut2[t] : 0xFFu;
    }
    if (STAGE && threadIdx.x < 2) {
        const uint32_t t = threadIdx.x;
        s_jump[2 * t] = reinterpret_cast<uint64_t>(ix.jump) + (t ? ix.jump_buckets * kJumpBucketBytes : 0u);   // (level 2 lies behind level 1)
        s_jump[2 * t + 1] = t ? ix.jump2_buckets : ix.jump_buckets;
        s_jump_k[t] = t ? ix.jump2_k : ix.jump_k;
    }
    RBG_RUN_SEARCH2_SHARED;
    const RunSearch2<P> S2 = stage_run_search2<P>(ix, s_tab_first, s_ent2, s_dir2, s_rec2, s_dyn);
    const uint32_t *tab_first = s_tab_first;
    lds_byte *tile = (lds_byte *)s_tile + (GLDS ? (threadIdx.x >> 6) * kTileBytes : 0u);   // (C-style: a cast into the LDS address space)
    if (PACKED || STAGE) {
        for (int t = threadIdx.x; t < 256; t += blockDim.x)
            if (s_lut2[t] != 0xFFu) s_mslot[s_lut2[t] & 3u] = s_lut[t];   // major index -> symbol slot
        __syncthreads();
    }
    const uint32_t D = ix.run_ksteps, DMASK = ix.run_depth_mask | 1u;
    const uint32_t M = ix.nmajor;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    lds_u32 *codes = (lds_u32 *)s_codes + (STAGE ? (threadIdx.x >> 6) * (kStageWords * 64u) + lane : 0u);   // this lane's column: word w at codes[64 w]
    const StageTab stage_tab{ix.stage_code[0], ix.stage_code[1], ix.stage_byte[0], ix.stage_byte[1], ix.stage_shift};
    const bool stage_on = STAGE && ix.stage_ok != 0 && M == 4;

    unsigned long long c_occ = 0, c_reads = 0;
    uint32_t c_matched = 0;
    unsigned long long st[kStatSearchN] = {0, 0, 0, 0, 0, 0, 0, 0};   // STATS only (dead code otherwise)
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const uint64_t wave_first = static_cast<uint64_t>(blockIdx.x) * blockDim.x + (threadIdx.x & ~(kWave - 1));
    for (uint64_t base = wave_first; base < Neff; base += stride) {  // the lanes of a wave iterate together
        bool valid = base + lane < Neff;
        const uint64_t i = (sel && valid) ? static_cast<uint64_t>(sel[base + lane]) : base + lane;
        uint64_t beg = 0, p = 0;
        PackedBits bs{chunks, make_uint4(0, 0, 0, 0), 4u, 0u, 0ull};
        if (PACKED) {
            if (valid) {
                const uint2 mt = meta[i];
                if (mt.y & 0x80000000u) valid = false;           // has a non-major symbol: the byte kernel answers it
                else { p = mt.y; bs.cp = chunks + mt.x; }        // p = symbols still to consume (beg = 0)
            }
        } else if (valid) { beg = off[i]; p = off[i + 1]; }
        // STAGE: the wave's reads become 2-bit codes in LDS (stage_read above) unless one of them is too long or holds a symbol outside the k-mer
        // alphabet; the walk below is instantiated for both forms, the wave takes one
        bool staged = false;
        if constexpr (STAGE && !PACKED) {
            if (stage_on && __ballot(valid && p - beg > kStageCap) == 0) {
                uint32_t nch = 0;
                const bool bad = valid && stage_read(reinterpret_cast<const uint4 *>(seqs), beg, p, stage_tab, codes, nch);
                if (STATS) st[kStChunks] += nch;
                staged = __ballot(bad) == 0;
                if (staged) { p -= beg; beg = 0; }
                else if (STATS) st[kStChunks] -= nch;          // (the byte walk counts its own)
            }
        }
        auto walk = [&](auto staged_tag) __attribute__((always_inline)) {
            constexpr bool STAGED = decltype(staged_tag)::value;
            const uint64_t p_end = p;
            uint64_t p_min = p;                                    // STATS: lowest read byte fetched
            const uint32_t m32 = static_cast<uint32_t>(p);         // STAGED: the read's length (p counts the symbols still to consume, beg = 0)
            uint64_t lo = 0, hi = ix.n - 1;                       // full_range(), rowbowt.hpp:115-118
            uint64_t k = TOEHOLD ? ix.last_run_sample : 0;
            bool alive = valid;
            bool pend = false;                                     // deferred toehold re-sample (k_search.hip): the last one is the only one used
            uint32_t pend_d = 0, pend_rec = 0;
            uint64_t pend_e = 0;
            ByteCursor rd{reinterpret_cast<const uint4 *>(seqs), ~uint64_t(0), make_uint4(0, 0, 0, 0)};
            // JUMP (rbg_jump.h): a staged read of at least jump_k symbols looks its last jump_k up in the table of the K-mers that occur -- one
            // probe in place of the ftab entry and the first (jump_k - ftab_k) / 8 steps; a key that is absent ends the read where its level is complete, and takes the ftab path below where it is not.
            // The probe is the wave's (jump_probe_wave): every lane enters it, `probing` is a predicate.
            bool jumped = false;
            if constexpr (STAGED && sizeof(P) == 4) {
                if (ix.jump) {                                     // (wave-uniform)
                    // Level 2 (ix.jump2_k): a lane that hit level 1 and has jump2_k symbols left looks {those symbols, its lo} up in the second
                    // table; a hit replaces the state once more; an absent key ends the read where level 2 is complete (below), and where it is not leaves level
                    // 1's state and the steps go on from there.  One loop over
                    // the levels: the probe is inlined once.
                    const uint32_t nlev = ix.jump2_k ? 2u : 1u;
                    bool hit = valid;                              // of the level before
                    uint32_t from = 0;                             // symbols the levels before consumed
#pragma unroll 1
                    for (uint32_t lev = 0; lev < nlev; ++lev) {
                        const uint32_t K = __builtin_amdgcn_readfirstlane(s_jump_k[lev]);
                        const uint64_t tab = uniform_u64(s_jump[2 * lev]), nb = uniform_u64(s_jump[2 * lev + 1]);
                        const bool probing = hit && static_cast<uint32_t>(p) >= K;
                        // level 1: the first jump_k symbols in consumption order; level 2: the jump2_k after them, and lo in the last word
                        JumpKey key = jump_key_from_codes(StagedWords{codes}, from, K);
                        if (lev) key.w[3] = static_cast<uint32_t>(lo);
                        from = K;
                        uint32_t v[3] = {0, 0, 0}, nbk = 0;
                        hit = jump_probe_wave<GLDS>(reinterpret_cast<const void *>(tab), nb, probing, key, v, nbk, tile);
                        if (hit) {
                            lo = v[0]; hi = v[1];
                            if (TOEHOLD) k = v[2] == 0xFFFFFFFFu ? ~uint64_t(0) : static_cast<uint64_t>(v[2]);
                            p -= K;
                            jumped = true;
                            if (STATS) st[kStSymbols] += K;
                        }
                        if (STATS) st[kStFtab] += nbk;               // (the ftab slot counts probed buckets too: 64 bytes each, of either level)
                        // A COMPLETE level (rbg_jump.h jump_complete_mask) holds every word that occurs, so a key it lacks ends the read here: its
                        // range is empty, the ftab path and the steps would only walk to the {1, 0, 0} below.  The argument needs the key to be one
                        // the enumeration could have reached, and it is: a wave is staged only if stage_read found none but major bytes in every
                        // read (stage_tables keeps one byte per major code and refuses every other), and k_jump.hip extends every word by exactly
                        // those four.  A predicate, not a way out of the loop: the next level's `hit` is false for this lane, the ballots of the
                        // probe and of the steps stay the wave's.  The instrumented kernel keeps walking: its sums describe the walk without this end.
                        if constexpr (!STATS) {
                            if (probing && !hit && jump_absent_ends(ix.jump_complete, lev)) { alive = false; p = beg; }
                        }
                    }
                }
            }
            if (!jumped && valid && ix.ftab_k && p - beg >= ix.ftab_k) {      // rowbowt.hpp:124-125, :745-758 (k_search.hip)
                uint64_t idx = 0;
                bool all_major = true;
                PackedBits probe = bs;                             // consumed only if the entry is usable
                if constexpr (STAGED) {
                    const uint32_t w0 = codes[0];                  // the first ftab_k (<= 16) symbols are the low 2 * ftab_k bits of the first word
                    idx = ix.ftab_k >= 16u ? w0 : (w0 & ((1u << (2u * ix.ftab_k)) - 1u));
                } else if (PACKED) {
                    idx = probe.take(2 * ix.ftab_k);               // the first ftab_k symbols are the low 2 * ftab_k bits
                } else {
                    uint64_t pw = 1;
                    for (uint32_t t = 1; t <= ix.ftab_k; ++t) {
                        const uint32_t mm = s_lut2[rd.at(p - t)];
                        all_major = all_major && mm != 0xFFu;
                        idx += (mm & 3u) * pw;
                        pw *= M;
                    }
                }
                uint64_t flo, fhi2, fk;
                if (STATS) { if (!STAGED) p_min = p - ix.ftab_k; if (all_major) st[kStFtab] += 1; }
                if (all_major && ftab_lookup<P>(ix, idx, flo, fhi2, fk)) {
                    if (PACKED) bs = probe;
                    lo = flo; hi = fhi2;
                    if (TOEHOLD) k = fk;
                    p -= ix.ftab_k;
                    if (STATS) st[kStSymbols] += ix.ftab_k;
                    if (hi < lo) { alive = false; p = beg; }
                }
            }
            // The steps of a read do not depend on the search: which table a step goes through is a matter of the read's symbols alone.  So the
            // NEXT step is chosen, and its table's record fetched (from LDS, or for depths 6-8 from the global array: an L2 round trip), while
            // the current step's bucket record is on its way -- the dependent chain of a step is its record (and, rarely, a scan), nothing else.
            struct Pick { uint32_t d, adv, rec; bool ok; };
            auto pick_at = [&](const uint64_t pp) __attribute__((always_inline)) -> Pick {        // the step that consumes the symbols ending at pp (exclusive: pp > beg)
                Pick s{0u, 1u, 0u, true};
                if constexpr (STAGED) {
                    s.adv = pp < D ? static_cast<uint32_t>(pp) : D;
                    s.adv = 32u - static_cast<uint32_t>(__clz(DMASK & ((2u << (s.adv - 1)) - 1u)));   // the deepest depth kept that fits
                    const uint32_t t0 = m32 - static_cast<uint32_t>(pp);                               // symbols consumed so far
                    const lds_u32 *cw = codes + (t0 >> 4) * 64u;
                    const uint32_t v = __builtin_amdgcn_alignbit(cw[64], cw[0], (t0 & 15u) * 2u) & ((1u << (2u * s.adv)) - 1u);
                    s.rec = run_record(tab_first, s.adv, s.adv == 1 ? static_cast<uint32_t>(s_mslot[v]) : v);
                    s.d = s.adv - 1;
                } else if (PACKED) {
                    s.adv = pp < D ? static_cast<uint32_t>(pp) : D;
                    s.adv = 32u - static_cast<uint32_t>(__clz(DMASK & ((2u << (s.adv - 1)) - 1u)));   // the deepest depth kept that fits
                    const uint32_t v = bs.take(2 * s.adv);
                    s.rec = run_record(tab_first, s.adv, s.adv == 1 ? static_cast<uint32_t>(s_mslot[v]) : v);
                    s.d = s.adv - 1;
                } else {
                    const uint64_t q = pp - 1;
                    const uint32_t c = rd.at(q);
                    if (STATS && q < p_min) p_min = q;
                    const uint32_t m0 = s_lut2[c];
                    uint32_t acc = m0;
                    if (m0 != 0xFFu) {                              // the longest run of major symbols among the next D (k_search.hip)
                        uint32_t pw = M, run_acc = m0;              // (of its prefixes, the longest whose depth has run lists)
    #pragma unroll 1
                        for (uint32_t t = 1; t < static_cast<uint32_t>(kMaxRunDepth); ++t) {
                            if (t >= D || q < beg + t) break;
                            const uint32_t mm = s_lut2[rd.at(q - t)];
                            if (STATS && q - t < p_min) p_min = q - t;
                            if (mm == 0xFFu) break;
                            run_acc += mm * pw;
                            pw *= M;
                            if ((DMASK >> t) & 1u) { s.adv = t + 1; acc = run_acc; }
                        }
                    }
                    if (s.adv == 1) {
                        const uint32_t slot = s_lut[c];
                        // symbol absent (f_[c] >= f_[c+1], rowbowt.hpp:76).  (An index with more than kLdsSyms symbols is
                        // never given this layout: upload() keeps the slot tables for it.)
                        if (slot == 0xFFu || slot >= static_cast<uint32_t>(kLdsSyms)) s.ok = false;
                        else s.rec = run_record(tab_first, 1u, slot);
                    } else {
                        s.d = s.adv - 1;
                        s.rec = run_record(tab_first, s.adv, acc);
                    }
                }
                return s;
            };
            // (the packed form keeps the step's choice at the top of the loop: the extra state of looking ahead sent it to scratch, and no kernel
            //  of this layout may spill -- tests/test_capi_host.py test_no_run_indexed_kernel_spills)
            constexpr bool AHEAD = !PACKED || STAGED;
            Pick cur{0u, 1u, 0u, false};
            RunHot Rcur{0, 0};
            if (AHEAD && alive && p > beg) {
                cur = pick_at(p);
                if (cur.ok) Rcur = load_run_tab<P>(S2, cur.d, cur.rec);
            }
            while (__ballot(alive && p > beg)) {                   // right-to-left over the reads (rowbowt.hpp:127-129, :175-181)
                bool stepping = alive && p > beg;
                if (!AHEAD && stepping) {
                    cur = pick_at(p);
                    if (cur.ok) Rcur = load_run_tab<P>(S2, cur.d, cur.rec);
                }
                if (stepping && !cur.ok) { alive = false; stepping = false; }
                const uint32_t d = cur.d, adv = cur.adv, rec = cur.rec;
                const RunHot R = Rcur;
                // the step after this one (taken only if this one leaves the range non-empty)
                const uint64_t p_next = p - adv;
                if (AHEAD && stepping && p_next > beg) {
                    cur = pick_at(p_next);
                    if (cur.ok) Rcur = load_run_tab<P>(S2, cur.d, cur.rec);
                }
                RunStep r;
                // rank(lo, c), rank(hi + 1, c): rowbowt.hpp:79,83
                lane_lf2_quad<P, STATS, false, GLDS>(S2, stepping, d, rec, R, lo, hi + 1, r, st, tile);   // (every lane of the wave: the records are fetched by quads)
                if (stepping) {
                    if (STATS) st[kStSymbols] += adv;
                    const uint64_t c_inside = r.c_upto - r.c_before;
                    if (c_inside == 0) {                            // rowbowt.hpp:85 (whichever of the nested steps emptied the range)
                        alive = false;
                    } else {
                        if (TOEHOLD) {                              // LF_w_loc, rowbowt.hpp:559-566, `adv` times nested
                            if (r.inside) k = k - adv;
                            else { pend = true; pend_d = d; pend_rec = rec; pend_e = r.samp_e; k = 0; }
                        }
                        lo = r.F + r.c_before;                      // rowbowt.hpp:86
                        hi = lo + c_inside - 1;                     // rowbowt.hpp:87
                        p = p_next;                                 // the left neighbours are consumed too
                    }
                }
            }
            if (TOEHOLD && alive && pend) {
                k += run_step_sample2<P>(ix, S2, pend_d, pend_rec, pend_e);
                if (STATS) st[kStResample] += 1;
            }
            if (STATS && !PACKED && !STAGED && p_end > p_min) st[kStChunks] += ((p_end - 1) >> 4) - (p_min >> 4) + 1;
            if (STATS && PACKED && valid) st[kStChunks] += (p_end + 63) >> 6;
            if (!alive) { lo = 1; hi = 0; k = 0; }                 // {1,0}; LFData::clear rowbowt.hpp:153-159
            if (valid) {
                lo_out[i] = lo;
                hi_out[i] = hi;
                if (TOEHOLD) ss_out[i] = k;
                c_reads += 1;
                if (alive) { c_matched += 1; c_occ += hi - lo + 1; }
            }
        };
        if (STAGE && staged) walk(std::integral_constant<bool, STAGE>{}); else walk(std::false_type{});
    }
    c_reads = wave_sum(c_reads);
    const unsigned long long w_matched = wave_sum(static_cast<unsigned long long>(c_matched));
    c_occ = wave_sum(c_occ);
    if (lane == 0 && c_reads) {
        atomicAdd(&ix.counters[0], c_reads);
        if (w_matched) atomicAdd(&ix.counters[1], w_matched);
        if (c_occ) atomicAdd(&ix.counters[2], c_occ);
    }
    if (STATS) {
#pragma unroll
        for (int t = 0; t < kStatSearchN; ++t) {
            const unsigned long long v = wave_sum(st[t]);
            if (lane == 0 && v) atomicAdd(&stats[t], v);
        }
    }
}

template <typename P> struct ChunkR { static constexpr int v = 8; };   // as in k_locate.hip (flush windows of eight locations: 64 bytes)

// ---- K3 over the run-indexed layout: ToeholdSA::locate_range (toehold_sa.hpp:37-49) -- every lane walks its own chain and
// answers its own phi (toehold_sa.hpp:56-72; rbg_runs2_device.hpp run_phi).  The chains, the staging of the values in LDS and
// the coalesced flush are k_locate_fill's: one body, rbg_chain_walk.hpp chain_fill_walk (chains in toehold order), its step
// loop not unrolled here (the phi step is long); a phi step is one directory
// gather (two neighbouring counts, plus the super count at 8-byte positions) and one scan of the bucket's few sampled
// positions, no cross-lane traffic.  Works for ordered and unordered walks alike (the order only decides how well
// neighbouring lanes share sectors).  STATS: [kLsPhiSteps] phi evaluations, [kLsPhiOvf] sampled positions the scans
// and the narrowing rounds needed (8 or 12 bytes each; 7 pivot keys per round), [kLsChains], [kLsLocs].
template <typename P, typename OUT = uint64_t, bool STATS = false, bool SUB = false, bool HI8 = false>
__global__ __launch_bounds__(256, 4) void k_locate_fill_runs2(const DevIndex ix, const uint64_t *__restrict__ lo,
                                                          const uint64_t *__restrict__ hi, const uint64_t *__restrict__ k,
                                                          const uint64_t N, const uint64_t max_hits,
                                                          const uint64_t *__restrict__ loc_off, OUT *__restrict__ locs,
                                                          const uint64_t *__restrict__ sub, const uint32_t *__restrict__ order,
                                                          const uint64_t *__restrict__ skeys, unsigned long long *__restrict__ stats) {
    constexpr int kChunkR = ChunkR<P>::v;
    using Stage = ChainStage<P, kChunkR, SUB, true, HI8>;
    __shared__ Stage S;   // (rbg_device.hpp: the staging and the flush are k_locate_fill's)
    chain_fill_walk<P, OUT, STATS, SUB, HI8, kChunkR, 1>(ix, S, lo, hi, k, N, max_hits, loc_off, locs, sub, order, skeys, stats,
                                                         [&](const uint64_t k1, unsigned long long &cost) { return run_phi<P, STATS>(ix, k1, cost); });
}

// ---- document hits from the walk itself (rbg_locate_docs.hpp) over the run-indexed layout's phi list: k_locate_fill_runs2's chains and its phi
// step (run_phi), the positions resolved and reduced instead of stored ----
extern __shared__ unsigned long long locate_docs_lds[];
template <typename P, bool LOCS>
__global__ __launch_bounds__(kLocDocBlock) void k_locate_docs_runs2(const DevIndex ix, const DocTable t, const uint64_t *__restrict__ lo,
                                                                   const uint64_t *__restrict__ hi, const uint64_t *__restrict__ k, const uint64_t N,
                                                                   const uint64_t max_hits, const uint32_t *__restrict__ order,
                                                                   const uint64_t *__restrict__ skeys, uint64_t *__restrict__ sets,
                                                                   uint32_t *__restrict__ ndocs_out, uint32_t *__restrict__ nodoc_out,
                                                                   unsigned long long *__restrict__ doc_reads, unsigned long long *__restrict__ doc_locs) {
    locate_docs_walk<P, LOCS>(ix, t, locate_docs_lds, lo, hi, k, N, max_hits, order, skeys, sets, ndocs_out, nodoc_out, doc_reads, doc_locs,
                              [&](const uint64_t k1, unsigned long long &cost) { return run_phi<P>(ix, k1, cost); });
}

}  // namespace

// `packed`: src_a = chunks, src_b = meta (see the kernel); stats != nullptr: the instrumented instantiation
int launch_find_range_runs_impl(const DevIndex &ix, const LaunchCfg &cfg, const void *src_a, const void *src_b, uint64_t N,
                                uint64_t *lo, uint64_t *hi, uint64_t *ssamp, void *stream, bool packed, unsigned long long *stats,
                                const uint32_t *sel = nullptr, const uint32_t *nsel = nullptr) {
    if (N == 0) return 0;
    const size_t lds = run_search2_lds(ix);
    // how a quad's bucket records travel (rbg_runs2_device.hpp): LDS-direct loads (the default), or RBG_REC_FETCH=quad: registers + quad permutes
    static const bool glds = [] { const char *e = std::getenv("RBG_REC_FETCH"); return !(e && std::strcmp(e, "quad") == 0); }();
    // the byte form stages its reads as 2-bit codes in LDS (STAGE above; needs an alphabet the register tables express: DevIndex::stage_ok);
    // RBG_STAGE_READS=0: every lane walks its read through a cursor of 16-byte chunks as before round 6 (A/B, profiles/r06_k2_sectors.md)
    static const bool stage = [] { const char *e = std::getenv("RBG_STAGE_READS"); return !(e && e[0] == '0'); }();
    if (stats && packed) return static_cast<int>(hipErrorNotSupported);
    const LaunchCfg c = runs512_cfg(cfg);
    // sel mode: the number of reads is only known on the device; a fixed modest grid loops over it
    const dim3 grid(sel ? std::min(grid_for(c, N), 256) : grid_for(c, N)), block(512);
    return with_pos(ix.pos_bytes, [&](auto p) { return with_flag(ssamp != nullptr, [&](auto toe) {
        auto search = [&](auto pk, auto sts, auto gl, auto sg) {
            constexpr bool GL = decltype(gl)::value, SG = decltype(sg)::value;
            return launch_lds(k_find_range_runs<pos_t<decltype(p)>, decltype(toe)::value, decltype(pk)::value, decltype(sts)::value, GL, SG>, grid, block, lds,
                              (GL ? 8 * kTileBytes : 0) + (SG ? 8 * kStageWaveBytes : 0), stream, ix, src_a, src_b, N, lo, hi, ssamp, stats, sel, nsel);
        };
        // the variants that exist: the byte form staged, LDS-direct or by quads (instrumented or not); the packed form LDS-direct or by quads
        auto fetch = [&](auto pk, auto sts) {
            if constexpr (!decltype(pk)::value) { if (glds && stage && !sel) return search(no, sts, yes, yes); }
            return glds ? search(pk, sts, yes, no) : search(pk, sts, no, no);
        };
        if (stats) return fetch(no, yes);
        return packed ? fetch(yes, no) : fetch(no, no);
    }); });
}

int launch_find_range_runs(const DevIndex &ix, const LaunchCfg &cfg, const uint8_t *seqs, const uint64_t *off, uint64_t N,
                           uint64_t *lo, uint64_t *hi, uint64_t *ssamp, void *stream, unsigned long long *stats) {
    return launch_find_range_runs_impl(ix, cfg, seqs, off, N, lo, hi, ssamp, stream, false, stats);
}

int launch_find_range_runs_sel(const DevIndex &ix, const LaunchCfg &cfg, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t *lo,
                               uint64_t *hi, uint64_t *ssamp, const uint32_t *sel, const uint32_t *nsel, void *stream) {
    return launch_find_range_runs_impl(ix, cfg, seqs, off, N, lo, hi, ssamp, stream, false, nullptr, sel, nsel);
}

int launch_find_range_runs_packed(const DevIndex &ix, const LaunchCfg &cfg, const uint2 *meta, const uint4 *chunks, uint64_t N,
                                  uint64_t *lo, uint64_t *hi, uint64_t *ssamp, void *stream) {
    return launch_find_range_runs_impl(ix, cfg, chunks, meta, N, lo, hi, ssamp, stream, true, nullptr);
}

int launch_locate_fill_runs(const DevIndex &ix, const LaunchCfg &cfg, const uint64_t *lo, const uint64_t *hi, const uint64_t *k,
                            uint64_t N, uint64_t max_hits, const uint64_t *loc_off, uint64_t *locs, const uint64_t *sub,
                            const void *order, const uint64_t *skeys, void *stream, unsigned long long *stats, uint32_t *locs32) {
    if (N == 0) return 0;
    const dim3 grid(grid_for(cfg, N)), block(256);
    const uint32_t *perm = static_cast<const uint32_t *>(order);
    return chain_fill_variants(ix, stats, sub, locs, locs32, [&](auto p, auto sts, auto sb, auto h8, auto *dst) {
        return launch_grid(k_locate_fill_runs2<pos_t<decltype(p)>, std::remove_pointer_t<decltype(dst)>, decltype(sts)::value, decltype(sb)::value, decltype(h8)::value>,
                           grid, block, 0, stream, ix, lo, hi, k, N, max_hits, loc_off, dst, sub, perm, skeys, stats);
    });
}

int launch_locate_doc_hits_runs(const DevIndex &ix, const DocTable &t, const uint64_t *lo, const uint64_t *hi, const uint64_t *k, uint64_t N, uint64_t max_hits,
                                const void *order, const uint64_t *skeys, uint64_t *sets, uint32_t *ndocs_out, uint32_t *nodoc_out, uint64_t *doc_reads,
                                uint64_t *doc_locs, void *stream) {
    if (t.ndocs == 0 || t.ndocs > kLocDocLdsDocs) return static_cast<int>(hipErrorInvalidValue);
    if (N == 0) return 0;
    const dim3 grid(locate_docs_grid(N)), block(kLocDocBlock);
    const uint32_t *perm = static_cast<const uint32_t *>(order);
    unsigned long long *dr = reinterpret_cast<unsigned long long *>(doc_reads), *dl = reinterpret_cast<unsigned long long *>(doc_locs);
    const size_t lds = locate_docs_lds_bytes(t.ndocs, t.ndir, doc_locs != nullptr);
    return with_pos(ix.pos_bytes, [&](auto p) { return with_flag(doc_locs != nullptr, [&](auto lc) {
        return launch_lds(k_locate_docs_runs2<pos_t<decltype(p)>, decltype(lc)::value>, grid, block, lds, 0, stream,
                          ix, t, lo, hi, k, N, max_hits, perm, skeys, sets, ndocs_out, nodoc_out, dr, dl);
    }); });
}

}  // namespace rbg
