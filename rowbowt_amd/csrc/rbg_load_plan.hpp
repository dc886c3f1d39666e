// rbg_load_plan.hpp -- what a load puts on the device, decided from plain numbers: the replica budget and its raise, the slot or run-indexed layout, the
// k-mer depths planned, kept and left out, which depths get bucket records, the ftab and the jump table's share -- and the GEOMETRY of the run-indexed
// layout: bucket shifts of directories and records, the uniform geometry of the deepest depth, the phi slots and the phi directory, the read-staging
// register tables.  capi/load.ipp (upload(), options_for()) and capi/upload_runs.ipp call these; nothing here reads the environment, an option, the device or an rbg_index, and nothing
// prints: the callers read those once, pass values in and say on stderr what was decided.  Plain host C++: tests/cpp/load_plan_check.cpp drives it alone.
#ifndef RBG_LOAD_PLAN_HPP
#define RBG_LOAD_PLAN_HPP

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rbg.h"
#include "rbg_host.hpp"
#include "rbg_jump.h"

namespace rbg {

// What the rules need of rbg_dev.h and the arena (that header is the device's: a host compiler does not take it).  capi/core.ipp load_consts() fills it.
struct LoadConsts {
    uint32_t max_narrow_shift, max_wide_shift;   // kMaxNarrowShift, kMaxWideShift
    uint32_t lds_syms;                           // kLdsSyms: the symbols the run-indexed layout serves
    size_t slot_bytes;                           // a rank slot and its ordinal: sizeof(RankSlot) + sizeof(uint32_t)
    size_t arena_align;                          // kArenaAlign
    size_t runs_samp_bytes[2], phi_ent_bytes[2]; // RunsFmt<P>::samp_bytes, PhiFmt<P>::ent_bytes at [0] 4-byte, [1] 8-byte positions
    uint32_t lds_run_depth;                      // kLdsRunDepth: the depths whose hot words are staged in LDS (a deeper one may be uniform)
    uint32_t uni_stride_bits, uni_shift_bits, uni_first_bits;   // rbg_runs2_device.hpp load_run_tab's packed constants of the uniform depth: 27, 5, 24
    uint32_t phi_packed_pos_bits, phi_packed_max_shift;         // kPhiPackedPosBits, kPhiPackedMaxShift
    size_t phi_slot_bytes[2], phi_slot_packed_bytes, phi_pair_bytes[2];   // sizeof(PhiSlot<P>), sizeof(PhiSlotPacked), sizeof(PhiEnt<P>)
};

// ---- the budget ----------------------------------------------------------------------------------------------------------------------------------
// The replica's share of the free HBM when no budget is given (RBG_OPT_HBM_BUDGET_MB): A QUARTER.  Until round 3 a default
// rbg_load took three quarters -- the bench index then got its 5-symbol slot level (218 GB) for the last 10-15 % of K1/K2's
// speed and left its caller 80 GB of a 288 GB device.  A drop-in library should leave the device to its caller unless told
// otherwise: with a quarter the same load keeps the 4-symbol level (58 GB), and the budget option is one call away.
inline size_t default_budget(size_t free_b) { return free_b / 4; }
// The budget of this load: the one options_for() fixed before anything of the load was on the device (plan_budget; 0: none), else the option, else the quarter.
inline size_t load_budget(size_t free_b, int64_t opt_mb, uint64_t plan_budget) {
    return plan_budget ? static_cast<size_t>(plan_budget) : opt_mb > 0 ? static_cast<size_t>(opt_mb) << 20 : default_budget(free_b);
}
// RBG_ASSUME_FREE_HBM_MB (tests only; read by capi/core.ipp): the free HBM the PLANNING of a load assumes (budget, composition depth), capped to this many
// MiB -- so that the rules an index of r = 1e9 runs meets on a 288 GB device (budget raised, depth planned before composing) are exercised by a test-sized
// index.  Allocation itself is not limited by it.
inline size_t assumed_free_hbm(size_t free_b, long long assumed_mb) {
    return assumed_mb <= 0 ? free_b : std::min<size_t>(free_b, static_cast<size_t>(assumed_mb) << 20);
}

// ---- the k-mer depths of the run-indexed layout --------------------------------------------------------------------------------------------------
// The k-mer depths that get run lists when RBG_OPT_RUN_DEPTHS names none: the deepest K, then K / 2, K / 4, ... and 1 (of eight: 1, 2, 4, 8).
// A search step consumes the longest stretch a kept depth covers, so whole reads go by K symbols a step and the remainder of a
// read (or of a seed) takes one step per set bit; every depth kept costs its run lists.
inline uint32_t default_depth_mask(uint32_t K) {
    uint32_t mask = 1u;
    for (uint32_t d = K; d >= 1; d /= 2) mask |= 1u << (d - 1);
    return mask;
}
inline uint32_t asked_depth_mask(int64_t run_depths_opt, uint32_t K) { return run_depths_opt ? static_cast<uint32_t>(run_depths_opt) | 1u : default_depth_mask(K); }
// How many symbols per step of the run-indexed layout are worth composing, estimated BEFORE composing: a depth adds at most about 0.62 r runs to
// the one before it (measured 0.55-0.69 r per depth at r = 1.07e9, n / r = 282; 0.33 r on the bench index), pieces are indexed with 32 bits, the
// sweeps hold about 70 bytes per piece of the depth being made (profiles/r04_pangenome_stream_r1e9_k5.log), and -- with_budget -- the least the budget
// rule of upload() keeps of a depth K (the single symbols, K itself, phi) must fit the budget at 18 bytes per entry.
inline double est_depth_runs(double r, uint32_t d) { return r * (1.0 + 0.62 * static_cast<double>(d - 1)); }
inline uint32_t planned_depth(double r, bool samples, uint32_t K0, double free_b, double budget, bool with_budget) {
    const double per_entry = 8.0 + (samples ? 6.0 : 0.0) + 4.0;
    uint32_t K = K0;
    while (K > 1) {
        bool ok = est_depth_runs(r, K) < 0.9 * 4294967296.0 && 70.0 * est_depth_runs(r, K) <= 0.95 * free_b;
        if (ok && with_budget) ok = (samples ? 16.0 * r : 0.0) + (est_depth_runs(r, 1) + est_depth_runs(r, K)) * per_entry <= budget;
        if (ok) break;
        --K;
    }
    return K;
}

// ---- slot tables or run lists --------------------------------------------------------------------------------------------------------------------
// the run-indexed layout is certain before anything is composed: asked for, or chosen by options_for() (rbg_index::auto_runs)
inline bool runs_certain(int64_t layout_opt, bool auto_runs) { return layout_opt == RBG_LAYOUT_RUNS || auto_runs; }
// the single-symbol slot level, estimated from n alone: a narrow-bucket table per symbol, phi at its widest usual bucket (64 rows)
inline double slot_level1_estimate(uint64_t n, uint32_t sigma, uint32_t pos_bytes, const LoadConsts &c) {
    return static_cast<double>(sigma) * static_cast<double>((n >> c.max_narrow_shift) + 2) * static_cast<double>(c.slot_bytes) +
           static_cast<double>((n >> 6) + 2) * (4.0 * pos_bytes + 4);
}
// the deepest level whose slot tables (every table at this bucket shift) fit the budget with the levels above it
inline int slot_levels_fitting(uint64_t n, double major, int slot_steps, uint32_t shift, double budget, const LoadConsts &c) {
    const double per_table = static_cast<double>((n >> shift) + 2) * static_cast<double>(c.slot_bytes);
    double total = major * per_table, tables = major;
    int keep = 1;
    for (int k = 2; k <= slot_steps; ++k) {
        tables *= major;
        total += tables * per_table;
        if (total > budget) break;
        keep = k;
    }
    return keep;
}
// the run-indexed replica at its leanest: about 110 bytes per run
inline bool runs_layout_fits(uint64_t r, double budget) { return 110.0 * static_cast<double>(r) <= budget; }

// An index so large that not even its single-symbol slot tables fit may also be too large for the DEFAULT budget to step by more than a symbol or two
// (r = 1e9: 36 GB of run lists and phi before any k-mer depth; profiles/r05_pangenome_stream_r1e9_default.json: 5e7 reads/s from the quarter, 1.4e8 from
// the fast form).  RBG_LAYOUT_AUTO with no budget given then takes up to three quarters of the free HBM -- and only on a device this load has (almost) to
// itself: with a tenth of it or more already taken (whole_b: the device's memory) -- the caller's own buffers, another replica, another process -- the
// quarter stays (a caller that sized its buffers around the quarter rule).  A raise that gains no depth is not made.
struct BudgetRaise {
    bool raise;
    double raised;   // three quarters of the free HBM
    uint32_t want;   // the symbols per step the quarter should have left
};
inline BudgetRaise budget_raise(double r, int kmer_steps, size_t free_b, size_t whole_b, int64_t opt_mb, int64_t layout_opt, double budget) {
    BudgetRaise b{false, 0.75 * static_cast<double>(free_b), static_cast<uint32_t>(std::min(kmer_steps, 4))};
    const bool device_to_itself = static_cast<double>(free_b) >= 0.9 * static_cast<double>(whole_b);
    const uint32_t K0 = static_cast<uint32_t>(kmer_steps);
    const uint32_t from_quarter = planned_depth(r, true, K0, static_cast<double>(free_b), budget, true);
    b.raise = opt_mb == 0 && layout_opt == RBG_LAYOUT_AUTO && device_to_itself && from_quarter < b.want &&
              planned_depth(r, true, K0, static_cast<double>(free_b), b.raised, true) > from_quarter;
    return b;
}

// ---- the geometry of the run-indexed layout ------------------------------------------------------------------------------------------------------
// What capi/upload_runs.ipp builds, as functions of plain numbers; the planner below estimates with the same functions.
// THE BUCKET SHIFT of a directory or of bucket records: the widest bucket that still holds at most `per` entries on average, at most 2^max_shift rows
// (31 at 4-byte positions; at 8-byte positions the fill shift: a bucket is no wider than the distance the fillers keep).  A table without runs counts as one.
inline uint32_t bucket_shift(double runs, double per, uint64_t n, uint32_t max_shift) {
    uint32_t sh = 0;
    runs = std::max(1.0, runs);
    while (sh < max_shift && runs * static_cast<double>(uint64_t(2) << sh) <= per * static_cast<double>(n)) ++sh;
    return sh;
}
inline uint64_t bucket_count(uint64_t n, uint32_t shift) { return (n >> shift) + 2; }

// UNIFORM geometry (rbg_dev.h DevIndex::run_uni_*) for a depth whose hot words a step would read from global memory: one shift -- the widest for the
// depth's AVERAGE table -- and one record count for every table, so that a step computes its table's hot word.  One depth can be uniform: the deepest kept
// one with records.  uni_switch (RBG_RUN_UNIFORM; tests, A/B): -1 the rules decide, 0 never, 1 whenever the depth is deep enough and the constants pack.
// (rec_per, mask, D: run_record_plan() below)
inline bool deepest_with_records(const std::vector<double> &rec_per, uint32_t mask, uint32_t d, uint32_t D) {
    for (uint32_t d2 = d + 1; d2 < D; ++d2)
        if ((mask >> d2 & 1u) && rec_per[d2] > 0) return false;
    return true;
}
inline bool uniform_stride_fits(uint64_t stride, const LoadConsts &c) { return !(stride >> c.uni_stride_bits); }
struct UniformCandidate {
    bool eligible;
    uint32_t shift;
    uint64_t stride;   // records per table
};
// The CANDIDATE, before anything is built: eligible when this is the deepest kept depth with records, deeper than the LDS-staged ones, with more than one
// table; its stride, shift and table ordinals fit load_run_tab's packed constants; and it costs no more than a tenth more records than the tables' own
// shifts (own_records) -- or the switch forces it.  tables_before: the tables of the shallower depths; total_runs: the entries of this depth's tables.
inline UniformCandidate uniform_candidate(bool deepest_recs, uint32_t depth_index, size_t tables, size_t tables_before, double total_runs, uint64_t own_records,
                                          double per, uint64_t n, uint32_t max_shift, int uni_switch, const LoadConsts &c) {
    UniformCandidate u{false, 0, 0};
    if (!(deepest_recs && depth_index >= c.lds_run_depth && uni_switch != 0 && tables > 1)) return u;
    u.shift = bucket_shift(total_runs / static_cast<double>(tables), per, n, max_shift);
    u.stride = bucket_count(n, u.shift);
    u.eligible = uniform_stride_fits(u.stride, c) && u.shift < (1u << c.uni_shift_bits) && tables_before + tables < (size_t(1) << c.uni_first_bits) &&
                 (uni_switch == 1 || static_cast<double>(u.stride) * static_cast<double>(tables) <= 1.1 * static_cast<double>(own_records));
    return u;
}
// The VERDICT, after the uniform records are built and their overflowing buckets counted (more than eleven entries: pivots + a scan of the run list, two
// or three sectors instead of one).  Those come from how a locus's runs cluster, whatever the geometry: on the bench index 4.9 % of the uniform depth-8
// records against 4.7 % under the tables' own shifts.  So a uniform depth with MANY of them (more than one record in 256; never when forced) is measured
// against the tables' own shifts, not against zero: it stays when it overflows at most a quarter more often -- a depth with a few very frequent k-mers
// keeps per-table shifts.
inline bool uniform_needs_comparison(uint64_t novf, uint64_t records, int uni_switch) {
    return uni_switch != 1 && static_cast<double>(novf) * 256.0 > static_cast<double>(records);
}
inline bool uniform_stays(uint64_t novf_uni, uint64_t novf_own, uint64_t records_uni) {
    return static_cast<double>(novf_uni) <= 1.25 * static_cast<double>(novf_own) + static_cast<double>(records_uni) / 256.0;
}

// PHI SLOTS on this layout (RBG_OPT_RUN_PHI = 2, or automatic): the slot layout's direct-addressed phi records with buckets of about n / r rows -- the
// widest bucket with at most one sampled position on average, at most 2^8 rows, never narrower than phi's own buckets (phi_shift) -- so that their number
// is proportional to r, not n.  Packed 16-byte slots at 8-byte positions while n and the shift allow (rbg_dev.h PhiSlotPacked).
struct PhiSlotBuckets {   // what depends on n, r and phi's own buckets alone: the planner's estimate needs no more
    uint32_t shift;
    uint64_t buckets;
};
inline PhiSlotBuckets phi_slot_buckets(uint64_t n, uint64_t r, uint32_t phi_shift) {
    PhiSlotBuckets b{0, 0};
    const double rows_per_sample = static_cast<double>(n) / static_cast<double>(std::max<uint64_t>(1, r));
    while (b.shift < 8 && static_cast<double>(uint64_t(2) << b.shift) <= rows_per_sample) ++b.shift;
    if (b.shift < phi_shift) b.shift = phi_shift;
    b.buckets = bucket_count(n, b.shift);
    return b;
}
struct PhiSlotGeometry {
    uint32_t shift;
    bool packed;
    size_t bucket_bytes;   // a slot and its 4-byte ordinal
    uint64_t buckets;
    size_t reserve;        // what the builder puts on the device: the buckets and the r + 1 {pos, base} pairs
    size_t slot_bytes() const { return bucket_bytes - 4; }
};
inline PhiSlotGeometry phi_slot_geometry(uint64_t n, uint64_t r, uint32_t phi_shift, uint32_t pos_bytes, const LoadConsts &c) {
    const PhiSlotBuckets b = phi_slot_buckets(n, r, phi_shift);
    PhiSlotGeometry g{b.shift, false, 0, b.buckets, 0};
    const bool wide = pos_bytes == 8;
    g.packed = wide && (n >> c.phi_packed_pos_bits) == 0 && g.shift <= c.phi_packed_max_shift;
    g.bucket_bytes = (g.packed ? c.phi_slot_packed_bytes : c.phi_slot_bytes[wide]) + 4;
    g.reserve = g.buckets * g.bucket_bytes + (r + 1) * c.phi_pair_bytes[wide];
    return g;
}
// phi by slots?  run_phi_opt (RBG_OPT_RUN_PHI): 2 yes, 1 no, 0 automatic: only while the slots are O(r) -- at most two buckets per sampled position (the
// bucket shift stops at 8: an index with n / r far beyond 256 would get n / 256 of them) -- and the whole replica stays within the budget (hbm_bytes: what
// the load has put on the device so far; the bucket records of the rank tables, decided before, have left room for the slots).
inline bool phi_by_slots(int64_t run_phi_opt, const PhiSlotGeometry &g, uint64_t r, uint64_t hbm_bytes, uint64_t hbm_budget) {
    return run_phi_opt == 2 || (run_phi_opt == 0 && hbm_budget && g.buckets <= 2 * r && hbm_bytes + g.reserve <= hbm_budget);
}
// THE PHI DIRECTORY over the list of sampled positions: the narrowest bucket (from 4 rows; at most 2^30, and 2^max_shift) with `per` sampled positions
// or more on average -- between per and 2 per (RBG_PHI_DIR_PER, default 1: the scan's first four requests then cover the bucket and its predecessor
// nineteen times in twenty).
inline uint32_t phi_dir_shift(uint64_t r, uint64_t n, double per, uint32_t max_shift) {
    uint32_t ds = 2;
    while (ds < max_shift && ds < 30 && (static_cast<double>(r) * static_cast<double>(uint64_t(1) << ds)) / static_cast<double>(n) < per) ++ds;
    return ds;
}
// THE REGISTER TABLES of the in-kernel read staging (rbg_dev.h stage_*): the least shift 0..5 under which the four major bytes hash to four different
// three-bit places; code[place] = the byte's major index, byte[place] = the byte.  An unused place must never equal the byte that hashes to it: it holds
// a byte whose own hash is another place.
struct StageTables {
    bool ok;
    uint32_t shift;
    uint8_t code[8], byte[8];
};
inline StageTables stage_tables(const uint8_t major_byte[4]) {
    StageTables s{false, 0, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};
    for (uint32_t sh = 0; sh <= 5 && !s.ok; ++sh) {
        uint8_t code[8] = {0, 0, 0, 0, 0, 0, 0, 0}, byte[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        bool used[8] = {false, false, false, false, false, false, false, false}, distinct = true;
        for (uint32_t m = 0; m < 4; ++m) {
            const uint32_t t = (major_byte[m] >> sh) & 7u;
            if (used[t]) distinct = false;
            used[t] = true;
            code[t] = static_cast<uint8_t>(m);
            byte[t] = major_byte[m];
        }
        if (!distinct) continue;
        for (uint32_t t = 0; t < 8; ++t)
            if (!used[t]) byte[t] = static_cast<uint8_t>(((t ^ 1u) & 7u) << sh);
        s.ok = true;
        s.shift = sh;
        std::copy(code, code + 8, s.code);
        std::copy(byte, byte + 8, s.byte);
    }
    return s;
}

// ---- the shape of an index: what the space rules of the run-indexed layout read of a HostIndex ----------------------------------------------------
struct IndexShape {
    uint64_t n = 0, r = 0;
    bool has_tsa = false;
    uint32_t pos_bytes = 4, phi_shift = 0;
    std::vector<uint64_t> nruns[kMaxKmerDepth];   // [d - 1]: the runs of each table of depth d (none: the depth has no tables)
};
inline IndexShape shape_of(const HostIndex &h) {
    IndexShape s;
    s.n = h.n; s.r = h.r; s.has_tsa = h.has_tsa; s.pos_bytes = h.pos_bytes; s.phi_shift = h.phi_shift;
    for (uint32_t di = 0; di < static_cast<uint32_t>(kMaxKmerDepth); ++di)
        for (const SymTable &t : di == 0 ? h.sym : h.kmer(di + 1)) s.nruns[di].push_back(t.nruns);
    return s;
}
inline uint64_t depth_entries(const IndexShape &s, uint32_t depth_index) {   // run-list entries of one depth: every table's runs and its sentinel
    uint64_t entries = 0;
    for (const uint64_t nr : s.nruns[depth_index]) entries += nr + 1;
    return entries;
}
// bytes of the run-indexed replica with the k-mer depths of `mask` (bit d - 1) among those the index holds (run lists, samples,
// 1/15 of sampled keys, phi)
inline size_t runs_replica_bytes(const IndexShape &s, const LoadConsts &c, uint32_t mask = ~0u) {
    size_t total = 0;
    const bool wide = s.pos_bytes == 8;
    // 8-byte entries at either width, directory entries of 4 / 8 bytes per (at most) half a run
    const size_t ent_bytes = 8, dir_per_entry = wide ? 4 : 2;
    for (uint32_t di = 0; di < static_cast<uint32_t>(kMaxKmerDepth); ++di) {
        if (!((mask | 1u) >> di & 1u)) continue;
        const size_t entries = depth_entries(s, di);
        total += entries * (ent_bytes + (s.has_tsa ? c.runs_samp_bytes[wide] : 0)) + entries * dir_per_entry + s.nruns[di].size() * 8 + 8 * c.arena_align;
    }
    if (s.has_tsa) total += (s.r + 1) * c.phi_ent_bytes[wide] + s.r * 4;   // (+ the phi directory: at most r entries)
    return total + 16 * c.arena_align;
}
// bucket records of one k-mer depth at `per` entries per bucket on average: their number (a sparse table's bucket shift stops at max_shift)
inline double runs_record_count(const IndexShape &s, uint32_t depth_index, double per, uint32_t max_shift) {
    double nrec = 0;
    for (const uint64_t nr : s.nruns[depth_index]) nrec += static_cast<double>(bucket_count(s.n, bucket_shift(static_cast<double>(nr), per, s.n, max_shift)));
    return nrec;
}
// phi slots of about n / r rows on the run-indexed layout: their bytes, or 0 where the automatic rule would not build them (more than 2 r buckets).
// The shift and the bucket count are the builder's (phi_slot_buckets), the bytes are not: THIS estimate differs from what the builder reserves
// (phi_slot_geometry): 36 / 20 bytes per bucket whatever the form -- where the builder packs (8-byte
// positions, n < 2^38, shift <= 6: 20 bytes) it is too high -- and without the r + 1 {pos, base} pairs.  The rules were moved, not changed.
inline double runs_phi_slot_bytes(const IndexShape &s) {
    if (!s.has_tsa) return 0;
    const double nb = static_cast<double>(phi_slot_buckets(s.n, s.r, s.phi_shift).buckets);
    return nb <= 2.0 * static_cast<double>(s.r) ? nb * (s.pos_bytes == 8 ? 36.0 : 20.0) : 0.0;
}
// what bucket records share the budget with: the replica, and the phi slots first (RBG_OPT_RUN_PHI = 1 builds none): their room is not the records'
inline double runs_bytes_before_records(const IndexShape &s, const LoadConsts &c, uint32_t mask, int64_t run_phi_opt) {
    double bytes = static_cast<double>(runs_replica_bytes(s, c, mask));
    if (run_phi_opt != 1) bytes += runs_phi_slot_bytes(s);
    return bytes;
}
constexpr double kRecBytes = 64.0;                  // one aligned record per bucket (rbg_dev.h RunRec2)
constexpr double kRecPers[3] = {2.5, 4.0, 6.0};     // entries per bucket on average: the narrowest first (a compact record holds eleven)

// ---- run-indexed layout over budget: which depths go -----------------------------------------------------------------------------------------------
// A step needs no table of every depth below the deepest -- a stretch of 4 symbols is a depth-3 step and a single one where depth 4 is left out -- and
// the deepest lists are the largest (2.4 entries per run at depth 5 of the H = 200 pangenome, 9.3 over the five).  Over budget the depths
// between the first and the deepest go first (deepest of them first), then the deepest itself; the new deepest depth is then stepped by again, and must
// still have its lists (a depth the composition gave back early goes too).  What is decided comes back as the steps to apply and to say, in order.
struct TrimStep {
    enum Kind { kLevelAboveMask, kLeaveOutDepth, kDropDeepest, kLevelWithoutData, kEndsOnly } kind;
    uint32_t depth;                 // the depth left out or dropped (kEndsOnly: the deepest kept)
    size_t tables;                  // kDropDeepest: the tables of that depth
    double need, with_ends;         // the replica that exceeded the budget (kEndsOnly: with records for every kept depth / for both ends)
    bool drops_level() const { return kind == kLevelAboveMask || kind == kDropDeepest || kind == kLevelWithoutData; }
};
struct RunTrim {
    uint32_t mask = 0, levels = 1, depths_dropped_budget = 0;
    std::vector<TrimStep> steps;
};
// asked_mask: asked_depth_mask(); levels: the deepest depth that has tables; has_data: bit d - 1 = depth d still has its run lists somewhere
inline RunTrim trim_run_depths(const IndexShape &s, const LoadConsts &c, uint32_t asked_mask, uint32_t levels, size_t budget, uint32_t has_data) {
    RunTrim t;
    t.mask = asked_mask;
    t.levels = levels;
    auto drop = [&](TrimStep::Kind kind, double need) { t.steps.push_back({kind, t.levels, s.nruns[t.levels - 1].size(), need, 0}); --t.levels; };
    while (t.levels > 1 && !(t.mask >> (t.levels - 1) & 1u)) drop(TrimStep::kLevelAboveMask, 0);   // (nothing steps by a depth above the deepest kept)
    t.mask &= (1u << t.levels) - 1u;
    // (depths above t.levels have no bit in the mask: the shape's lists of a level that went are not counted)
    for (size_t need; (need = runs_replica_bytes(s, c, t.mask)) > budget && t.levels > 1;) {
        uint32_t mid = 0;
        for (uint32_t d = t.levels - 1; d >= 2 && !mid; --d)
            if (t.mask >> (d - 1) & 1u) mid = d;
        if (mid) {
            t.steps.push_back({TrimStep::kLeaveOutDepth, mid, 0, static_cast<double>(need), 0});
            t.mask &= ~(1u << (mid - 1));
            t.depths_dropped_budget |= 1u << (mid - 1);
            continue;
        }
        t.depths_dropped_budget |= 1u << (t.levels - 1);
        drop(TrimStep::kDropDeepest, static_cast<double>(need));
        while (t.levels > 1 && !(has_data >> (t.levels - 1) & 1u)) drop(TrimStep::kLevelWithoutData, 0);
        t.mask = (t.mask & ((1u << t.levels) - 1u)) | (1u << (t.levels - 1));   // (the new deepest level is stepped by again)
    }
    return t;
}
// Records everywhere before depths in between: a depth whose ranks go through a directory pays narrowing rounds in crowded buckets (n = 5e10 under the
// default budget: 2.7 rounds and 78 scanned entries per read, K2 13.8 ms against 7 with records; profiles/r05_pangenome_stream_n5e10_default.json),
// the depths between the first and the deepest save a step per read.  So when the automatic rules decide (no RBG_OPT_RUN_DEPTHS, no RBG_OPT_RUN_REC) and
// bucket records for every kept depth do not fit the budget, but would with the first and the deepest depth alone, the depths between them go.
inline bool ends_only_rule_applies(int64_t run_depths_opt, int64_t run_rec_opt, uint32_t levels) { return run_depths_opt == 0 && run_rec_opt == 0 && levels > 2; }
inline void trim_to_ends_for_records(const IndexShape &s, const LoadConsts &c, RunTrim &t, size_t budget, uint32_t max_shift, int64_t run_phi_opt) {
    const uint32_t ends = 1u | (1u << (t.levels - 1));
    auto with_records = [&](uint32_t m) {
        double bytes = runs_bytes_before_records(s, c, m, run_phi_opt);
        for (uint32_t d = 0; d < t.levels; ++d)
            if (m >> d & 1u) bytes += runs_record_count(s, d, kRecPers[2], max_shift) * kRecBytes;
        return bytes;
    };
    if (t.mask != ends && with_records(t.mask) > static_cast<double>(budget) && with_records(ends) <= static_cast<double>(budget)) {
        t.steps.push_back({TrimStep::kEndsOnly, t.levels, 0, with_records(t.mask), with_records(ends)});
        t.depths_dropped_budget |= t.mask & ~ends;
        t.mask = ends;
    }
}

// ---- bucket records per depth (RBG_OPT_RUN_REC; rbg_dev.h RunRec2) ---------------------------------------------------------------------------------
// PER DEPTH, deepest first (a search spends its steps at the deepest depth; the shallower ones take a read's ragged ends): rec_per[d] = entries per
// bucket on average of depth d's records, 0 = directories.  RBG_OPT_RUN_REC = 2: the depths of RBG_OPT_RUN_REC_DEPTHS (0 = all kept) at RBG_RUN_REC_PER
// (rec_asked; 0: 2.5).  Automatic (0, and a budget known): each depth in turn gets the narrowest buckets -- 2.5, 4 or 6 entries -- with which the replica
// (phi slots included) stays within the budget and the records stay O(r) (at most one per entry).  D: the depths composed; mask: those with run lists.
inline std::vector<double> run_record_plan(const IndexShape &s, const LoadConsts &c, uint32_t mask, uint32_t D, uint64_t hbm_budget, int64_t run_rec_opt,
                                           int64_t run_rec_depths_opt, double rec_asked, uint32_t max_shift, int64_t run_phi_opt) {
    std::vector<double> rec_per(D, 0.0);
    if (run_rec_opt == 2) {
        const uint32_t want = run_rec_depths_opt ? static_cast<uint32_t>(run_rec_depths_opt) : ~0u;
        for (uint32_t d = 0; d < D; ++d)
            if ((mask >> d & 1u) && (want >> d & 1u)) rec_per[d] = rec_asked > 0 ? rec_asked : kRecPers[0];
    } else if (run_rec_opt == 0 && hbm_budget) {
        double total = runs_bytes_before_records(s, c, mask, run_phi_opt);
        const double budget = static_cast<double>(hbm_budget);
        // room at the widest buckets (6 entries) for EVERY kept depth?  Then every depth gets records -- a depth left on directories pays narrowing rounds on
        // its steps -- and a depth takes narrower buckets only with what the shallower ones do not need.  Otherwise: deepest first, while they fit.
        std::vector<double> widest(D, 0.0), entries(D, 0.0);
        double all_widest = 0;
        bool every = true;
        for (uint32_t d = 0; d < D; ++d) {
            if (!(mask >> d & 1u)) continue;
            entries[d] = static_cast<double>(depth_entries(s, d));
            widest[d] = runs_record_count(s, d, rec_asked > 0 ? rec_asked : kRecPers[2], max_shift) * kRecBytes;
            all_widest += widest[d];
            every = every && widest[d] <= entries[d] * kRecBytes;
        }
        every = every && total + all_widest <= budget;
        double shallower_widest = all_widest;
        for (int d = static_cast<int>(D) - 1; d >= 0; --d) {
            if (!(mask >> d & 1u)) continue;
            shallower_widest -= widest[d];
            for (const double per : kRecPers) {
                if (rec_asked > 0 && per != kRecPers[0]) break;
                const double use = rec_asked > 0 ? rec_asked : per;
                const double bytes = runs_record_count(s, static_cast<uint32_t>(d), use, max_shift) * kRecBytes;
                if (bytes <= entries[d] * kRecBytes && total + bytes + (every ? shallower_widest : 0.0) <= budget) {
                    rec_per[d] = use;
                    total += bytes;
                    break;
                }
            }
        }
    }
    return rec_per;
}

// ---- the small rules -------------------------------------------------------------------------------------------------------------------------------
// Slot layout over budget: a k-mer table goes to the widest bucket that still holds about half a run start on average, at most 2^max_wide_shift rows, in
// the wide-slot encoding of rbg_dev.h (2^shift <= rows per run / 2); never narrower than it is, and not at all where wide slots cannot carry the ranks
// (40 bits).
inline uint32_t widened_shift(uint64_t n, uint64_t nruns, uint32_t shift, const LoadConsts &c) {
    if (n >> 40) return shift;
    const double rows_per_run = static_cast<double>(n) / static_cast<double>(std::max<uint64_t>(1, nruns));
    uint32_t want = 0;
    while (want < c.max_wide_shift && static_cast<double>(uint64_t(2) << want) <= rows_per_run) ++want;
    return std::max(want, shift);
}
// the automatic ftab: the longest word <= 12 with nmajor^k <= n/16 (4^12 words x 16 B = 268 MB; DESIGN.md 4 on why not longer)
inline int64_t auto_ftab_k(uint32_t nmajor, uint64_t n) {
    int64_t fk = 0;
    double w = 1;
    while (nmajor >= 2 && fk < 12 && w * nmajor <= static_cast<double>(n) / 16) { w *= nmajor; ++fk; }
    return fk;
}
inline double ftab_words(uint32_t nmajor, int64_t fk) {
    double words = 1;
    for (int64_t t = 0; t < fk; ++t) words *= nmajor;
    return words;
}
inline size_t ftab_entry_bytes(uint32_t pos_bytes) { return pos_bytes == 4 ? 16 : 32; }
// the table plus the scratch of building it (in chunks) must leave half of the free memory to the queries
inline bool ftab_fits(double words, size_t entry_bytes, size_t scratch_bytes, size_t free_b) {
    return words < 4.0e9 && words * static_cast<double>(entry_bytes) + static_cast<double>(scratch_bytes) < 0.5 * static_cast<double>(free_b);
}
// the jump table: automatic once the replica outgrows the last-level cache
inline int64_t auto_jump_k(uint64_t hbm_bytes) { return hbm_bytes > kJumpAutoMinBytes ? kJumpDefaultK : 0; }
// what the HBM budget leaves after the replica holds the build at its peak (scratch + table), and at most half of the free memory; by default the table
// may add at most half of the replica: on a text of few repeats -- nearly every K-mer distinct -- it would outgrow the index it serves (the bench index's
// is a third)
// Level 2 comes after level 1 and changes nothing of its rule: the first table is decided as if there were no second.  The two TOGETHER may
// take what the budget leaves and at most half of the free memory (the build's peak, scratch included, stays within that too); by default
// they may add at most the replica itself -- the bench index's two are three quarters of it.
struct JumpBudgets {
    uint64_t room, peak_budget, table_budget, both_budget;
};
inline JumpBudgets jump_budgets(uint64_t hbm_budget, uint64_t hbm_bytes, size_t free_b, bool jump_auto) {
    JumpBudgets j;
    j.room = hbm_budget > hbm_bytes ? hbm_budget - hbm_bytes : 0;
    j.peak_budget = std::min<uint64_t>(j.room, free_b / 2);
    j.table_budget = std::min<uint64_t>(j.room, free_b / 4);
    j.both_budget = j.peak_budget;
    if (jump_auto) {
        j.table_budget = std::min<uint64_t>(j.table_budget, hbm_bytes / 2);
        j.both_budget = std::min<uint64_t>(j.both_budget, hbm_bytes);
    }
    return j;
}
// level 2: asked for (16..48), or automatic -- 40 symbols where level 1 is the automatic one at its default of 60 (60 + 40 = 100), none otherwise
inline int64_t jump2_k_for(int64_t opt, bool jump_auto, int64_t jk) {
    if (opt >= 0) return opt;
    return jump_auto && jk == static_cast<int64_t>(kJumpDefaultK) ? static_cast<int64_t>(kJump2DefaultK) : 0;
}

}  // namespace rbg
#endif
