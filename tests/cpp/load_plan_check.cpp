// load_plan_check.cpp -- the load rules of rbg_load_plan.hpp and its geometry of the run-indexed layout as functions of plain numbers, checked on the CPU (tests/test_load_plan_host.py builds this
// with ASan + UBSan).  Every expectation is worked out by hand from the rule as its comment states it, or comes from a committed record: the arguments are
// the rows of tools/layout_rules_table.py DEFAULT, six numbers each: n r hbm_free_at_load hbm_budget budget_raised symbols_per_gather.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../rowbowt_amd/csrc/rbg_load_plan.hpp"

using namespace rbg;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// rbg_dev.h: kMaxNarrowShift 8, kMaxWideShift 12, kLdsSyms 8, a 16-byte slot and its 4-byte ordinal, 64 KB arena alignment, samples of 4 / 6 bytes, phi
// entries of 8 / 12 bytes; kLdsRunDepth 5, the uniform depth's packed constants of 27, 5 and 24 bits; packed phi slots up to 38-bit positions and shift 6; phi
// slots of 16 / 32 bytes, 16 packed; {pos, base} pairs of 8 / 16 bytes
static const LoadConsts C{8, 12, 8, 20, 65536, {4, 6}, {8, 12}, 5, 27, 5, 24, 38, 6, {16, 32}, 16, {8, 16}};
static const size_t kAlign8 = 8 * 65536, kAlign16 = 16 * 65536;

// n = 2^20, no samples, 4-byte positions; depth 1: tables of 99 and 199 runs (300 entries with their sentinels), depth 2: 49 (50), depth 3: 9 (10),
// depth 4: 19 (20).  A depth costs 10 bytes per entry (8 + 2 of directory), 8 per table and 8 alignments; the replica 16 alignments more.
static IndexShape four_depths() {
    IndexShape s;
    s.n = uint64_t(1) << 20; s.r = 1000; s.has_tsa = false; s.pos_bytes = 4; s.phi_shift = 0;
    s.nruns[0] = {99, 199}; s.nruns[1] = {49}; s.nruns[2] = {9}; s.nruns[3] = {19};
    return s;
}
static const size_t D1 = 300 * 10 + 16 + kAlign8, D2 = 50 * 10 + 8 + kAlign8, D3 = 10 * 10 + 8 + kAlign8, D4 = 20 * 10 + 8 + kAlign8;
// bucket records at 6 entries per bucket (64 bytes each; the bucket shift grows while runs * 2^(shift + 1) <= 6 n):
//   99 runs: shift 15, 34 records; 199: shift 14, 66; 49: shift 16, 18; 9: shift 19, 4; 19: shift 18, 6
static const double R1 = 100 * 64, R2 = 18 * 64, R3 = 4 * 64, R4 = 6 * 64;

static bool same_steps(const RunTrim &t, std::vector<TrimStep::Kind> kinds, std::vector<uint32_t> depths) {
    if (t.steps.size() != kinds.size()) return false;
    for (size_t i = 0; i < kinds.size(); ++i)
        if (t.steps[i].kind != kinds[i] || t.steps[i].depth != depths[i]) return false;
    return true;
}

static void check_rows(int argc, char **argv) {
    for (int a = 1; a + 5 < argc; a += 6) {
        const uint64_t r = std::strtoull(argv[a + 1], nullptr, 10), free_b = std::strtoull(argv[a + 2], nullptr, 10), budget = std::strtoull(argv[a + 3], nullptr, 10);
        const int raised = std::atoi(argv[a + 4]);
        const uint32_t symbols = static_cast<uint32_t>(std::atoi(argv[a + 5]));
        // every row was loaded with eight symbols asked for, no budget given, RBG_LAYOUT_AUTO, on a device it had to itself
        const size_t quarter = load_budget(free_b, 0, 0);
        const BudgetRaise b = budget_raise(static_cast<double>(r), 8, free_b, free_b, 0, RBG_LAYOUT_AUTO, static_cast<double>(quarter));
        CHECK(b.raise == (raised != 0));
        CHECK((raised ? static_cast<uint64_t>(b.raised) : static_cast<uint64_t>(quarter)) == budget);
        CHECK(planned_depth(static_cast<double>(r), true, 8, static_cast<double>(free_b), static_cast<double>(budget), true) == symbols);
        if (raised) CHECK(planned_depth(static_cast<double>(r), true, 8, static_cast<double>(free_b), static_cast<double>(quarter), true) == 2);   // (below the 4 wanted)
    }
}

static void check_budget_and_layout() {
    const uint32_t masks[8] = {0x01, 0x03, 0x05, 0x0B, 0x13, 0x25, 0x45, 0x8B};
    for (uint32_t K = 1; K <= 8; ++K) CHECK(default_depth_mask(K) == masks[K - 1]);
    CHECK(asked_depth_mask(0, 8) == 0x8B && asked_depth_mask(0x14, 8) == 0x15);
    CHECK(load_budget(1000, 0, 0) == 250 && load_budget(1000, 3, 0) == (size_t(3) << 20) && load_budget(1000, 3, 777) == 777);
    CHECK(assumed_free_hbm(size_t(5) << 20, 0) == (size_t(5) << 20) && assumed_free_hbm(size_t(5) << 20, -1) == (size_t(5) << 20));
    CHECK(assumed_free_hbm(size_t(5) << 20, 2) == (size_t(2) << 20) && assumed_free_hbm(size_t(1) << 20, 2) == (size_t(1) << 20));
    CHECK(runs_certain(RBG_LAYOUT_RUNS, false) && runs_certain(RBG_LAYOUT_AUTO, true) && !runs_certain(RBG_LAYOUT_AUTO, false) && !runs_certain(RBG_LAYOUT_SLOTS, false));
    // n = 2^16, five symbols: 5 tables of 256 + 2 slots of 20 bytes, phi: 1024 + 2 slots of 4 positions and a word
    CHECK(slot_level1_estimate(65536, 5, 4, C) == 5 * 258 * 20 + 1026 * 20);
    CHECK(slot_level1_estimate(65536, 5, 8, C) == 5 * 258 * 20 + 1026 * 36);
    // n = 0: 2 slots of 20 bytes per table; 4, 16, 64, 256, 1024 tables: 160, 800, 3360, 13600, 54560 bytes with the levels above
    CHECK(slot_levels_fitting(0, 4, 5, 12, 54560, C) == 5 && slot_levels_fitting(0, 4, 5, 12, 54559, C) == 4);
    CHECK(slot_levels_fitting(0, 4, 5, 12, 800, C) == 2 && slot_levels_fitting(0, 4, 5, 12, 799, C) == 1 && slot_levels_fitting(0, 4, 5, 12, 0, C) == 1);
    CHECK(slot_levels_fitting(0, 4, 1, 12, 1e9, C) == 1 && slot_levels_fitting(0, 4, 1, 12, 0, C) == 1);
    CHECK(slot_levels_fitting(uint64_t(1) << 20, 4, 5, 8, 4 * 4098 * 20, C) == 1 && slot_levels_fitting(uint64_t(1) << 20, 4, 5, 8, 20 * 4098 * 20, C) == 2);
    CHECK(runs_layout_fits(1000, 110000) && !runs_layout_fits(1000, 109999));
    // the raise: r = 1 068 485 643 on 288 GiB free.  A quarter (77.3 GB) holds depth 2 of the 4 wanted (16 r + 18 r (2 + 0.62 (K - 1)) bytes: 67.5 GB at
    // K = 2, 79.4 at 3); three quarters are not what limits it: depth 6 would have 4.38e9 pieces, more than 0.9 x 2^32 -- depth 5.
    const double r = 1068485643.0;
    const size_t whole = size_t(10) << 35, free9 = size_t(9) << 35;   // 0.9 x whole exactly
    const double quarter = static_cast<double>(free9 / 4);
    CHECK(planned_depth(r, true, 8, static_cast<double>(free9), quarter, true) == 2 && planned_depth(r, true, 8, static_cast<double>(free9), 0.75 * free9, true) == 5);
    const BudgetRaise yes = budget_raise(r, 8, free9, whole, 0, RBG_LAYOUT_AUTO, quarter);
    CHECK(yes.raise && yes.raised == 0.75 * static_cast<double>(free9) && yes.want == 4);
    CHECK(!budget_raise(r, 8, free9 - 1, whole, 0, RBG_LAYOUT_AUTO, static_cast<double>((free9 - 1) / 4)).raise);   // a byte less than nine tenths: not to itself
    CHECK(!budget_raise(r, 8, free9, whole, 70000, RBG_LAYOUT_AUTO, 70000.0 * 1048576).raise);                      // a budget given
    CHECK(!budget_raise(r, 8, free9, whole, 0, RBG_LAYOUT_PREFER_SLOTS, quarter).raise && !budget_raise(r, 8, free9, whole, 0, RBG_LAYOUT_RUNS, quarter).raise);
    CHECK(budget_raise(r, 3, free9, whole, 0, RBG_LAYOUT_AUTO, quarter).want == 3);
    // no depth gained: r = 1e9 on 110 GB free -- the sweeps of depth 2 (70 bytes x 1.62e9 pieces = 113.4 GB) do not fit 0.95 x 110 GB whatever the budget
    CHECK(planned_depth(1e9, true, 8, 1.1e11, 0.75 * 1.1e11, true) == 1);
    CHECK(!budget_raise(1e9, 8, size_t(110000000000), size_t(110000000000), 0, RBG_LAYOUT_AUTO, 1.1e11 / 4).raise);
}

static void check_space() {
    const IndexShape s = four_depths();
    CHECK(depth_entries(s, 0) == 300 && depth_entries(s, 3) == 20 && depth_entries(s, 4) == 0);
    CHECK(runs_replica_bytes(s, C, 0xF) == D1 + D2 + D3 + D4 + kAlign16 && runs_replica_bytes(s, C, 0x9) == D1 + D4 + kAlign16);
    CHECK(runs_replica_bytes(s, C, 0x8) == D1 + D4 + kAlign16);   // (depth 1 is always there)
    CHECK(runs_replica_bytes(s, C, 0xF) == 3149568);
    IndexShape w = s;   // with samples at 8-byte positions: 8 + 6 + 4 bytes per entry, phi: r + 1 entries of 12 bytes and r of directory
    w.has_tsa = true; w.pos_bytes = 8;
    CHECK(runs_replica_bytes(w, C, 0x1) == 300 * 18 + 16 + kAlign8 + 1001 * 12 + 4000 + kAlign16);
    CHECK(runs_record_count(s, 0, 6.0, 31) == 100 && runs_record_count(s, 1, 6.0, 31) == 18 && runs_record_count(s, 2, 6.0, 31) == 4 && runs_record_count(s, 3, 6.0, 31) == 6);
    CHECK(runs_record_count(s, 0, 6.0, 4) == 2 * ((s.n >> 4) + 2));   // the shift stops at max_shift
    CHECK(runs_record_count(s, 3, 2.5, 31) == 10);                    // 19 runs at 2.5 per bucket: shift 17, 8 + 2 records
    // phi slots: n / r = 1048.6 rows per run: the shift stops at 8 -- 4096 + 2 buckets, more than 2 r = 2000: none.  r = 3000: 20 / 36 bytes each.
    CHECK(runs_phi_slot_bytes(s) == 0 && runs_phi_slot_bytes(w) == 0);
    w.r = 3000;
    CHECK(runs_phi_slot_bytes(w) == 4098 * 36.0);
    w.pos_bytes = 4; w.phi_shift = 9;   // never narrower than phi's own buckets
    CHECK(runs_phi_slot_bytes(w) == 2050 * 20.0);
    w.has_tsa = false;
    CHECK(runs_phi_slot_bytes(w) == 0);
}

static void check_trimming() {
    const IndexShape s = four_depths();
    const size_t all = D1 + D2 + D3 + D4 + kAlign16;
    typedef TrimStep T;
    RunTrim t = trim_run_depths(s, C, 0xF, 4, all, 0xF);   // fits exactly: the test is >
    CHECK(t.mask == 0xF && t.levels == 4 && t.depths_dropped_budget == 0 && t.steps.empty());
    t = trim_run_depths(s, C, 0xF, 4, all - 1, 0xF);       // a byte short: the deepest of the depths in between goes
    CHECK(t.mask == 0xB && t.levels == 4 && t.depths_dropped_budget == 0x4 && same_steps(t, {T::kLeaveOutDepth}, {3}) && t.steps[0].need == static_cast<double>(all));
    t = trim_run_depths(s, C, 0xF, 4, all - D3 - 1, 0xF);   // then the next one
    CHECK(t.mask == 0x9 && t.levels == 4 && t.depths_dropped_budget == 0x6 && same_steps(t, {T::kLeaveOutDepth, T::kLeaveOutDepth}, {3, 2}));
    CHECK(t.steps.size() == 2 && t.steps[1].need == static_cast<double>(all - D3));
    // a byte less than depths 1 and 4 need: the deepest goes, and depth 3 -- left out a moment ago -- is the deepest now and stepped by again
    t = trim_run_depths(s, C, 0xF, 4, D1 + D4 + kAlign16 - 1, 0xF);
    CHECK(t.mask == 0x5 && t.levels == 3 && t.depths_dropped_budget == 0xE && same_steps(t, {T::kLeaveOutDepth, T::kLeaveOutDepth, T::kDropDeepest}, {3, 2, 4}));
    CHECK(t.steps.size() == 3 && t.steps[2].tables == 1 && t.steps[2].need == static_cast<double>(D1 + D4 + kAlign16));
    // the same with depth 3 given back by the composition: it is swept, depth 2 is the deepest; 1 and 2 need more than 1 and 4 did: depth 2 goes too
    t = trim_run_depths(s, C, 0xF, 4, D1 + D4 + kAlign16 - 1, 0xB);
    CHECK(t.mask == 0x1 && t.levels == 1 && t.depths_dropped_budget == 0xE);
    CHECK(same_steps(t, {T::kLeaveOutDepth, T::kLeaveOutDepth, T::kDropDeepest, T::kLevelWithoutData, T::kDropDeepest}, {3, 2, 4, 3, 2}));
    CHECK(t.steps.size() == 5 && t.steps[4].need == static_cast<double>(D1 + D2 + kAlign16));
    // nothing steps by a depth above the deepest asked for: those levels go without a word, whatever the budget; depth 1 stays whatever the budget
    t = trim_run_depths(s, C, 0x3, 4, size_t(1) << 40, 0xF);
    CHECK(t.mask == 0x3 && t.levels == 2 && t.depths_dropped_budget == 0 && same_steps(t, {T::kLevelAboveMask, T::kLevelAboveMask}, {4, 3}));
    t = trim_run_depths(s, C, 0x1, 1, 0, 0x1);
    CHECK(t.mask == 0x1 && t.levels == 1 && t.steps.empty());
    for (const T &st : std::vector<T>{{T::kLevelAboveMask, 2, 0, 0, 0}, {T::kDropDeepest, 2, 0, 0, 0}, {T::kLevelWithoutData, 2, 0, 0, 0}}) CHECK(st.drops_level());
    CHECK(!(T{T::kLeaveOutDepth, 2, 0, 0, 0}).drops_level() && !(T{T::kEndsOnly, 2, 0, 0, 0}).drops_level());

    // the ends-only rule: only the automatic rules, only with a depth in between
    CHECK(ends_only_rule_applies(0, 0, 3) && !ends_only_rule_applies(0, 0, 2) && !ends_only_rule_applies(0x1F, 0, 4) && !ends_only_rule_applies(0, 2, 4) && !ends_only_rule_applies(0, 1, 4));
    const double with_all = static_cast<double>(all) + R1 + R2 + R3 + R4, with_ends = static_cast<double>(D1 + D4 + kAlign16) + R1 + R4;
    t = trim_run_depths(s, C, 0xF, 4, all, 0xF);
    trim_to_ends_for_records(s, C, t, all, 31, 0);   // the run lists fit, their records do not, those of depths 1 and 4 alone would
    CHECK(t.mask == 0x9 && t.levels == 4 && t.depths_dropped_budget == 0x6 && same_steps(t, {T::kEndsOnly}, {4}));
    CHECK(t.steps.size() == 1 && t.steps[0].need == with_all && t.steps[0].with_ends == with_ends);
    t = trim_run_depths(s, C, 0xF, 4, static_cast<size_t>(with_all), 0xF);
    trim_to_ends_for_records(s, C, t, static_cast<size_t>(with_all), 31, 0);   // records for every depth fit exactly
    CHECK(t.mask == 0xF && t.depths_dropped_budget == 0 && t.steps.empty());
    t = trim_run_depths(s, C, 0xF, 4, static_cast<size_t>(with_all) - 1, 0xF);
    trim_to_ends_for_records(s, C, t, static_cast<size_t>(with_all) - 1, 31, 0);
    CHECK(t.mask == 0x9 && t.depths_dropped_budget == 0x6);
    // the default set of four depths (1, 2, 4) at the budget its run lists need: depth 2 goes for the records of 1 and 4
    t = trim_run_depths(s, C, default_depth_mask(4), 4, D1 + D2 + D4 + kAlign16, 0xF);
    trim_to_ends_for_records(s, C, t, D1 + D2 + D4 + kAlign16, 31, 0);
    CHECK(t.mask == 0x9 && t.depths_dropped_budget == 0x2 && same_steps(t, {T::kEndsOnly}, {4}));
    // already the two ends (after the budget took the depths between): nothing more to say
    t = trim_run_depths(s, C, 0xF, 4, D1 + D4 + kAlign16, 0xF);
    trim_to_ends_for_records(s, C, t, D1 + D4 + kAlign16, 31, 0);
    CHECK(t.mask == 0x9 && t.depths_dropped_budget == 0x6 && same_steps(t, {T::kLeaveOutDepth, T::kLeaveOutDepth}, {3, 2}));
    // records capped at shift 4 (65538 per table) fit with neither set: the depths stay
    t = trim_run_depths(s, C, 0xF, 4, all, 0xF);
    trim_to_ends_for_records(s, C, t, all, 4, 0);
    CHECK(t.mask == 0xF && t.steps.empty());
}

static bool same(const std::vector<double> &got, std::vector<double> want) { return got == want; }

static void check_records() {
    const IndexShape s = four_depths();
    const uint64_t all = D1 + D2 + D3 + D4 + kAlign16, widest = static_cast<uint64_t>(R1 + R2 + R3 + R4);   // 8192 bytes of records at 6 entries per bucket
    // records at 2.5 entries per bucket: depth 4: 10 (640 bytes), depth 3: 6 (384), depth 2: 34 (2176), depth 1: 66 + 130 (12544); at 4: 10, 6, 18, 34 + 66
    CHECK(same(run_record_plan(s, C, 0xF, 4, uint64_t(1) << 40, 0, 0, 0, 31, 0), {2.5, 2.5, 2.5, 2.5}));   // all the room: the narrowest everywhere
    // exactly the room for every depth at 6: every depth gets records; depth 4 and 3 at 6 (384 and 256 bytes: their 640 and 384 at 2.5 or 4 would take what
    // the shallower depths need), depths 2 and 1 at 4, where they have the 18 and 100 records they have at 6
    CHECK(same(run_record_plan(s, C, 0xF, 4, all + widest, 0, 0, 0, 31, 0), {4.0, 4.0, 6.0, 6.0}));
    // 256 bytes more: depth 4 takes them for its 640 bytes at 2.5
    CHECK(same(run_record_plan(s, C, 0xF, 4, all + widest + 256, 0, 0, 0, 31, 0), {4.0, 4.0, 6.0, 2.5}));
    // no room for all at 6 (1000 bytes): deepest first while they fit -- depth 4 at 2.5 (640), depth 3 at 6 (256 of the 360 left), then nothing fits
    CHECK(same(run_record_plan(s, C, 0xF, 4, all + 1000, 0, 0, 0, 31, 0), {0.0, 0.0, 6.0, 2.5}));
    CHECK(same(run_record_plan(s, C, 0xF, 4, all, 0, 0, 0, 31, 0), {0.0, 0.0, 0.0, 0.0}));
    // depths without run lists get none, and do not count
    CHECK(same(run_record_plan(s, C, 0x9, 4, D1 + D4 + kAlign16 + 6400 + 384, 0, 0, 0, 31, 0), {4.0, 0.0, 0.0, 6.0}));
    // RBG_OPT_RUN_REC = 2: the kept depths, or those of RBG_OPT_RUN_REC_DEPTHS among them, at 2.5 or RBG_RUN_REC_PER -- whatever the budget
    CHECK(same(run_record_plan(s, C, 0xB, 4, 0, 2, 0, 0, 31, 0), {2.5, 2.5, 0.0, 2.5}));
    CHECK(same(run_record_plan(s, C, 0xB, 4, 1, 2, 0xC, 0, 31, 0), {0.0, 0.0, 0.0, 2.5}));
    CHECK(same(run_record_plan(s, C, 0xB, 4, 1, 2, 0, 9.0, 31, 0), {9.0, 9.0, 0.0, 9.0}));
    // RBG_RUN_REC_PER with the automatic rule: that width or none
    CHECK(same(run_record_plan(s, C, 0xF, 4, uint64_t(1) << 40, 0, 0, 3.0, 31, 0), {3.0, 3.0, 3.0, 3.0}));
    // off, and automatic without a budget
    CHECK(same(run_record_plan(s, C, 0xF, 4, uint64_t(1) << 40, 1, 0, 0, 31, 0), {0.0, 0.0, 0.0, 0.0}));
    CHECK(same(run_record_plan(s, C, 0xF, 4, 0, 0, 0, 0, 31, 0), {0.0, 0.0, 0.0, 0.0}));
    // records that would outnumber the entries (the shift capped at 4: 65538 per table): none, whatever the room
    CHECK(same(run_record_plan(s, C, 0xF, 4, uint64_t(1) << 40, 0, 0, 0, 4, 0), {0.0, 0.0, 0.0, 0.0}));
    // ... for the one depth where they would: depth 1 with a table of 2^18 runs more has 262445 entries and 3 x 65538 records at shift 4, depth 4 has 20 and 65538
    IndexShape big = s;
    big.nruns[0].push_back(uint64_t(1) << 18);
    CHECK(same(run_record_plan(big, C, 0x9, 4, uint64_t(1) << 40, 0, 0, 0, 4, 0), {2.5, 0.0, 0.0, 0.0}));
    // phi slots come first: with samples, r = 3000 and 8-byte positions they take 4098 x 36 bytes of the room (RBG_OPT_RUN_PHI = 1: no slots)
    IndexShape w = s;
    w.has_tsa = true; w.pos_bytes = 8; w.r = 3000;
    const uint64_t base = runs_replica_bytes(w, C, 0x9);
    CHECK(same(run_record_plan(w, C, 0x9, 4, base + 6400 + 384, 0, 0, 0, 31, 1), {4.0, 0.0, 0.0, 6.0}));
    CHECK(same(run_record_plan(w, C, 0x9, 4, base + 6400 + 384, 0, 0, 0, 31, 0), {0.0, 0.0, 0.0, 0.0}));
    CHECK(same(run_record_plan(w, C, 0x9, 4, base + 4098 * 36 + 6400 + 384, 0, 0, 0, 31, 0), {4.0, 0.0, 0.0, 6.0}));
}

static void check_small_rules() {
    const uint64_t n = uint64_t(1) << 20;
    // 2^shift <= rows per run / 2, at most 2^12
    CHECK(widened_shift(n, 256, 0, C) == 12 && widened_shift(n, 257, 0, C) == 11 && widened_shift(n, 1, 0, C) == 12);
    CHECK(widened_shift(n, n / 2, 5, C) == 5 && widened_shift(n, n / 2, 0, C) == 1 && widened_shift(n, n, 0, C) == 0 && widened_shift(n, 0, 0, C) == 12);
    CHECK(widened_shift(uint64_t(1) << 40, 1, 3, C) == 3 && widened_shift((uint64_t(1) << 40) - 1, 1, 3, C) == 12);   // wide slots carry 40-bit ranks
    // nmajor^k <= n / 16, at most 12
    CHECK(auto_ftab_k(4, uint64_t(16) << 24) == 12 && auto_ftab_k(4, (uint64_t(16) << 24) - 1) == 11 && auto_ftab_k(4, uint64_t(16) << 40) == 12);
    CHECK(auto_ftab_k(4, 64) == 1 && auto_ftab_k(4, 63) == 0 && auto_ftab_k(1, n) == 0 && auto_ftab_k(2, 64) == 2);
    CHECK(ftab_words(4, 12) == 16777216.0 && ftab_words(3, 2) == 9.0 && ftab_entry_bytes(4) == 16 && ftab_entry_bytes(8) == 32);
    CHECK(ftab_fits(3999999999.0, 16, 0, size_t(1) << 40) && !ftab_fits(4.0e9, 16, 0, size_t(1) << 40));   // fewer than 4e9 words
    CHECK(!ftab_fits(1000, 16, 1000, 34000) && ftab_fits(1000, 16, 1000, 34002) && !ftab_fits(1000, 16, 1002, 34002));   // table + scratch < half the free memory
    CHECK(auto_jump_k(uint64_t(256) << 20) == 0 && auto_jump_k((uint64_t(256) << 20) + 1) == 60);
    JumpBudgets j = jump_budgets(1000, 400, 10000, false);
    CHECK(j.room == 600 && j.peak_budget == 600 && j.table_budget == 600);
    j = jump_budgets(1000, 400, 1000, false);   // at most half of the free memory at the peak, a quarter for the table
    CHECK(j.room == 600 && j.peak_budget == 500 && j.table_budget == 250);
    j = jump_budgets(400, 1000, 10000, false);
    CHECK(j.room == 0 && j.peak_budget == 0 && j.table_budget == 0);
    j = jump_budgets(3100, 2000, 10000, true);   // automatic: at most half the replica
    CHECK(j.room == 1100 && j.peak_budget == 1100 && j.table_budget == 1000);
    j = jump_budgets(3100, 2000, 10000, false);
    CHECK(j.table_budget == 1100);
    j = jump_budgets(2900, 2000, 10000, true);
    CHECK(j.table_budget == 900);
}


// ---- the geometry of the run-indexed layout ----------------------------------------------------------------------------------------------------------
static void check_bucket_shift() {
    const uint64_t n = uint64_t(1) << 20;
    // the shift grows while runs * 2^(shift + 1) <= per * n.  One run, one entry per bucket: 2^(shift + 1) <= 2^20 up to shift 19 -- shift 20; no run counts as one
    CHECK(bucket_shift(1, 1, n, 31) == 20 && bucket_shift(0, 1, n, 31) == 20 && bucket_shift(0.25, 1, n, 31) == 20);
    // four runs: 4 x 2^18 = 2^20 is still <= n (shift 18); with a row less it is not (17); five runs: 5 x 2^18 > 2^20 (17)
    CHECK(bucket_shift(4, 1, n, 31) == 18 && bucket_shift(4, 1, n - 1, 31) == 17 && bucket_shift(5, 1, n, 31) == 17);
    CHECK(bucket_shift(4, 2, n, 31) == 19 && bucket_shift(n, 1, n, 31) == 0 && bucket_shift(static_cast<double>(n / 2), 1, n, 31) == 1 && bucket_shift(static_cast<double>(n / 2 + 1), 1, n, 31) == 0);   // (n / 2 runs: 2 x n / 2 <= n)
    // the numbers of the record checks above: 99 runs at 6 per bucket: 15, 199: 14, 19 at 2.5: 17
    CHECK(bucket_shift(99, 6, n, 31) == 15 && bucket_shift(199, 6, n, 31) == 14 && bucket_shift(19, 2.5, n, 31) == 17);
    // it stops at max_shift: 31 at 4-byte positions, the fill shift (30, or a test's 5) at 8-byte positions
    CHECK(bucket_shift(1, 1e12, n, 31) == 31 && bucket_shift(1, 1e12, n, 30) == 30 && bucket_shift(1, 6, n, 5) == 5 && bucket_shift(1, 6, n, 0) == 0);
    CHECK(bucket_count(n, 15) == 34 && bucket_count(n, 31) == 2 && bucket_count(0, 0) == 2);
    // runs_record_count: the sum of (n >> shift) + 2 over the tables -- shifts 15 and 14; a table without runs (shift 20 at one per bucket) has 1 + 2
    IndexShape s = four_depths();
    CHECK(runs_record_count(s, 0, 6.0, 31) == static_cast<double>(((n >> 15) + 2) + ((n >> 14) + 2)));
    s.nruns[4] = {0, 1, 4};
    CHECK(runs_record_count(s, 4, 1.0, 31) == 3 + 3 + 6);
    CHECK(runs_record_count(s, 4, 1.0, 5) == 3 * ((n >> 5) + 2));
}

static void check_uniform() {
    const uint64_t n = uint64_t(1) << 20;
    // deepest_with_records: no deeper KEPT depth has records
    const std::vector<double> rec_per{2.5, 0.0, 4.0, 6.0};
    CHECK(deepest_with_records(rec_per, 0xF, 3, 4) && !deepest_with_records(rec_per, 0xF, 2, 4) && deepest_with_records(rec_per, 0x7, 2, 4) && !deepest_with_records(rec_per, 0xF, 0, 4));
    CHECK(deepest_with_records({2.5, 0.0, 0.0, 0.0}, 0xF, 0, 4));
    // four tables of depth index 5 with 16 entries together at one per bucket: the average table's shift is 18 (4 x 2^18 <= 2^20), 4 + 2 records per table,
    // 24 in all: at most 1.1 x the tables' own records when those are 22 (24.2), not when 21 (23.1)
    UniformCandidate u = uniform_candidate(true, 5, 4, 100, 16, 22, 1, n, 31, -1, C);
    CHECK(u.eligible && u.shift == 18 && u.stride == 6);
    CHECK(!uniform_candidate(true, 5, 4, 100, 16, 21, 1, n, 31, -1, C).eligible);
    // eleven tables: 66 records = 1.1 x 60 exactly: at most a tenth more; 59: more
    CHECK(uniform_candidate(true, 5, 11, 100, 44, 60, 1, n, 31, -1, C).eligible && !uniform_candidate(true, 5, 11, 100, 44, 59, 1, n, 31, -1, C).eligible);
    // each condition off alone: a deeper depth has records; a depth staged in LDS (index 4 = depth 5); forbidden; a single table
    CHECK(!uniform_candidate(false, 5, 4, 100, 16, 22, 1, n, 31, -1, C).eligible && !uniform_candidate(true, 4, 4, 100, 16, 22, 1, n, 31, -1, C).eligible);
    CHECK(!uniform_candidate(true, 5, 4, 100, 16, 22, 1, n, 31, 0, C).eligible && !uniform_candidate(true, 5, 1, 100, 4, 22, 1, n, 31, -1, C).eligible);
    CHECK(!uniform_candidate(true, 5, 4, 100, 16, 1000, 1, n, 31, 0, C).eligible && !uniform_candidate(true, 5, 1, 100, 4, 1, 1, n, 31, 1, C).eligible);
    CHECK(uniform_candidate(true, 7, 2, 0, 8, 22, 1, n, 31, -1, C).eligible);
    // forced: whatever the cost ...
    u = uniform_candidate(true, 5, 4, 100, 16, 1, 1, n, 31, 1, C);
    CHECK(u.eligible && u.shift == 18 && u.stride == 6 && !uniform_candidate(true, 5, 4, 100, 16, 1, 1, n, 31, -1, C).eligible);
    CHECK(!uniform_candidate(true, 4, 4, 100, 16, 1, 1, n, 31, 1, C).eligible && !uniform_candidate(false, 5, 4, 100, 16, 1, 1, n, 31, 1, C).eligible);
    // ... but not whatever the packing.  The stride (shift 0: n + 2 records per table) fits 27 bits at 2^27 - 1, not at 2^27
    const uint64_t n27 = (uint64_t(1) << 27) - 3;
    u = uniform_candidate(true, 5, 4, 100, 16, 1, 1, n27, 0, 1, C);
    CHECK(u.eligible && u.shift == 0 && u.stride == (uint64_t(1) << 27) - 1 && uniform_stride_fits(u.stride, C));
    u = uniform_candidate(true, 5, 4, 100, 16, 1, 1, n27 + 1, 0, 1, C);
    CHECK(!u.eligible && u.stride == uint64_t(1) << 27 && !uniform_stride_fits(u.stride, C));
    CHECK(uniform_candidate(true, 5, 4, 100, 16, uint64_t(1) << 40, 1, n27, 0, -1, C).eligible && !uniform_candidate(true, 5, 4, 100, 16, uint64_t(1) << 40, 1, n27 + 1, 0, -1, C).eligible);
    // the shift in 5 bits: 31 fits, 32 (no position width has it: a max_shift only this check passes) does not
    CHECK(uniform_candidate(true, 5, 4, 100, 4, 1, 1e30, n, 31, 1, C).eligible && uniform_candidate(true, 5, 4, 100, 4, 1, 1e30, n, 31, 1, C).shift == 31);
    CHECK(!uniform_candidate(true, 5, 4, 100, 4, 1, 1e30, n, 32, 1, C).eligible);
    // the tables up to and with this depth in 24 bits: 2^24 - 1 of them fit, 2^24 do not
    CHECK(uniform_candidate(true, 5, 4, (size_t(1) << 24) - 5, 16, 22, 1, n, 31, -1, C).eligible && !uniform_candidate(true, 5, 4, (size_t(1) << 24) - 4, 16, 22, 1, n, 31, -1, C).eligible);
    CHECK(!uniform_candidate(true, 5, 4, (size_t(1) << 24) - 4, 16, 22, 1, n, 31, 1, C).eligible);
    // the verdict after counting.  Compared at all: more than one record in 256 overflows (4 x 256 = 1024: not of 1024, of 1023 yes), never when forced
    CHECK(!uniform_needs_comparison(4, 1024, -1) && uniform_needs_comparison(4, 1023, -1) && !uniform_needs_comparison(0, 0, -1) && uniform_needs_comparison(1, 255, -1));
    CHECK(!uniform_needs_comparison(4, 1023, 1) && !uniform_needs_comparison(1000000, 1, 1));
    // uniform stays: at most a quarter more overflowing than the tables' own 8, and 512 / 256: 10 + 2 = 12
    CHECK(uniform_stays(12, 8, 512) && !uniform_stays(13, 8, 512) && uniform_stays(0, 0, 0) && !uniform_stays(1, 0, 255) && uniform_stays(1, 0, 256) && uniform_stays(5, 4, 0) && !uniform_stays(6, 4, 0));
}

static void check_phi_geometry() {
    const uint64_t r = 1024;
    // the shift grows while 2^(shift + 1) <= n / r, up to 8.  n / r = 1: 0; 2: 1; 255: 7 (256 > 255); 256: 8; 1e6: 8
    PhiSlotGeometry g = phi_slot_geometry(r, r, 0, 4, C);
    CHECK(g.shift == 0 && !g.packed && g.bucket_bytes == 20 && g.slot_bytes() == 16 && g.buckets == 1026 && g.reserve == 1026 * 20 + 1025 * 8);
    g = phi_slot_geometry(2 * r, r, 0, 4, C);
    CHECK(g.shift == 1 && g.buckets == 1026);
    g = phi_slot_geometry(255 * r, r, 0, 4, C);
    CHECK(g.shift == 7 && g.buckets == 2040 + 2 && phi_by_slots(0, g, r, 0, uint64_t(1) << 40));
    g = phi_slot_geometry(256 * r, r, 0, 4, C);
    CHECK(g.shift == 8 && g.buckets == 1026 && phi_by_slots(0, g, r, 0, uint64_t(1) << 40));
    g = phi_slot_geometry(1000000 * r, r, 0, 4, C);
    CHECK(g.shift == 8 && g.buckets == 4000000 + 2 && !phi_by_slots(0, g, r, 0, uint64_t(1) << 40) && phi_by_slots(2, g, r, 0, 0));
    // at most 2 r buckets: n = 2 r x 256 - 512 has 2 r - 2 + 2 of them, 256 rows more one too many
    g = phi_slot_geometry(2 * r * 256 - 512, r, 0, 4, C);
    CHECK(g.shift == 8 && g.buckets == 2 * r && phi_by_slots(0, g, r, 0, uint64_t(1) << 40));
    g = phi_slot_geometry(2 * r * 256 - 256, r, 0, 4, C);
    CHECK(g.buckets == 2 * r + 1 && !phi_by_slots(0, g, r, 0, uint64_t(1) << 40));
    // never narrower than phi's own buckets
    g = phi_slot_geometry(2 * r, r, 5, 4, C);
    CHECK(g.shift == 5 && g.buckets == 64 + 2);
    g = phi_slot_geometry(256 * r, r, 5, 4, C);
    CHECK(g.shift == 8);
    // packed: 8-byte positions, n < 2^38, shift <= 6.  n / r = 64: shift 6 -- 16 + 4 bytes per bucket, pairs of 16 bytes
    g = phi_slot_geometry(64 * r, r, 0, 8, C);
    CHECK(g.shift == 6 && g.packed && g.bucket_bytes == 20 && g.buckets == 1026 && g.reserve == 1026 * 20 + 1025 * 16);
    g = phi_slot_geometry(64 * r, r, 0, 4, C);    // 4-byte positions
    CHECK(g.shift == 6 && !g.packed && g.bucket_bytes == 20 && g.reserve == 1026 * 20 + 1025 * 8);
    g = phi_slot_geometry(128 * r, r, 0, 8, C);   // shift 7
    CHECK(g.shift == 7 && !g.packed && g.bucket_bytes == 36 && g.slot_bytes() == 32 && g.buckets == 1026 && g.reserve == 1026 * 36 + 1025 * 16);
    g = phi_slot_geometry(32 * r, r, 7, 8, C);    // phi's own shift 7
    CHECK(g.shift == 7 && !g.packed);
    const uint64_t r33 = uint64_t(1) << 33;       // n = 2^38 - 1 and 2^38 over 2^33 runs: 32 rows per sample (shift 5), phi's own shift 6
    g = phi_slot_geometry((uint64_t(1) << 38) - 1, r33, 6, 8, C);
    CHECK(g.shift == 6 && g.packed && g.buckets == (uint64_t(1) << 32) - 1 + 2);
    g = phi_slot_geometry(uint64_t(1) << 38, r33, 6, 8, C);
    CHECK(g.shift == 6 && !g.packed && g.bucket_bytes == 36 && g.buckets == (uint64_t(1) << 32) + 2);
    // phi_by_slots: 2 always, 1 never; automatic: a budget known, the buckets O(r), and what is on the device with the slots within the budget
    g = phi_slot_geometry(64 * r, r, 0, 8, C);
    CHECK(phi_by_slots(2, g, r, uint64_t(1) << 40, 1) && !phi_by_slots(1, g, r, 0, uint64_t(1) << 40) && !phi_by_slots(0, g, r, 0, 0));
    CHECK(phi_by_slots(0, g, r, 5000, 5000 + g.reserve) && !phi_by_slots(0, g, r, 5001, 5000 + g.reserve));
    // the planner's estimate for this shape, where the builder packs: 36 bytes per bucket, not the builder's 20, and no pairs
    IndexShape w;
    w.n = 64 * r; w.r = r; w.has_tsa = true; w.pos_bytes = 8; w.phi_shift = 0;
    CHECK(runs_phi_slot_bytes(w) == 1026 * 36.0 && g.buckets * g.bucket_bytes == 1026 * 20);
    w.pos_bytes = 4;
    CHECK(runs_phi_slot_bytes(w) == 1026 * 20.0);
    w.n = 2 * r * 256 - 256;   // one bucket more than 2 r: none
    CHECK(runs_phi_slot_bytes(w) == 0);
    w.n = 2 * r * 256 - 512;
    CHECK(runs_phi_slot_bytes(w) == 2048 * 20.0);

    // the phi directory: from shift 2, while r 2^shift / n < per; at most 30 and max_shift
    const uint64_t n = uint64_t(1) << 20;
    CHECK(phi_dir_shift(n, n, 1, 31) == 2 && phi_dir_shift(4 * n, n, 1, 31) == 2 && phi_dir_shift(n / 4, n, 1, 31) == 2 && phi_dir_shift(n / 4 - 1, n, 1, 31) == 3);
    CHECK(phi_dir_shift(1024, n, 1, 31) == 10 && phi_dir_shift(1023, n, 1, 31) == 11 && phi_dir_shift(1024, n, 2, 31) == 11 && phi_dir_shift(1024, n, 0.5, 31) == 9);
    CHECK(phi_dir_shift(1, uint64_t(1) << 40, 1, 31) == 30 && phi_dir_shift(1, uint64_t(1) << 40, 1, 12) == 12 && phi_dir_shift(1, uint64_t(1) << 40, 1, 5) == 5);
    CHECK(phi_dir_shift(1, uint64_t(1) << 40, 1, 1) == 2 && phi_dir_shift(1, uint64_t(1) << 40, 1, 2) == 2 && phi_dir_shift(1, uint64_t(1) << 29, 1, 31) == 29);
}

// the least shift 0..5 under which the four bytes' three-bit places differ, by brute force; -1: none
static int separating_shift(const uint8_t b[4]) {
    for (int sh = 0; sh <= 5; ++sh) {
        bool distinct = true;
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j) distinct = distinct && ((b[i] >> sh) & 7) != ((b[j] >> sh) & 7);
        if (distinct) return sh;
    }
    return -1;
}
static bool stage_tables_right(const uint8_t b[4]) {
    const StageTables s = stage_tables(b);
    const int want = separating_shift(b);
    if (!s.ok) return want < 0;
    if (want < 0 || s.shift != static_cast<uint32_t>(want)) return false;
    for (int v = 0; v < 256; ++v) {   // byte[place of v] == v exactly for the four major bytes, and code[...] is then the byte's major index
        int major = -1;
        for (int m = 0; m < 4; ++m)
            if (b[m] == v) major = m;
        const uint32_t place = (static_cast<uint32_t>(v) >> s.shift) & 7u;
        if ((s.byte[place] == v) != (major >= 0)) return false;
        if (major >= 0 && s.code[place] != major) return false;
    }
    return true;
}
static void check_stage_tables() {
    const uint8_t ACGT[4] = {'A', 'C', 'G', 'T'}, acgt[4] = {'a', 'c', 'g', 't'}, TGCA[4] = {'T', 'G', 'C', 'A'};
    CHECK(stage_tables_right(ACGT) && stage_tables(ACGT).ok && stage_tables(ACGT).shift == 0);   // A, C, G, T & 7: 1, 3, 7, 4
    CHECK(stage_tables(ACGT).code[1] == 0 && stage_tables(ACGT).code[3] == 1 && stage_tables(ACGT).code[7] == 2 && stage_tables(ACGT).code[4] == 3);
    CHECK(stage_tables_right(acgt) && stage_tables(acgt).ok && stage_tables(acgt).shift == 0 && stage_tables_right(TGCA) && stage_tables(TGCA).code[4] == 0);
    // 0x00, 0x08, 0x10, 0x18: the same place at shift 0, 0 4 0 4 at shift 1, 0 2 4 6 at shift 2
    const uint8_t later[4] = {0x00, 0x08, 0x10, 0x18};
    CHECK(stage_tables_right(later) && stage_tables(later).ok && stage_tables(later).shift == 2);
    // 0x00, 0x01, 0x80, 0x81: 0 1 0 1 at shift 0, four zeros at shifts 1..4, 0 0 4 4 at shift 5
    const uint8_t none[4] = {0x00, 0x01, 0x80, 0x81};
    CHECK(stage_tables_right(none) && !stage_tables(none).ok && separating_shift(none) < 0);
    std::mt19937 rng(20240229);
    int ok = 0, not_ok = 0, wrong = 0;
    for (int i = 0; i < 20000; ++i) {
        uint8_t b[4];
        for (int k = 0; k < 4;) {   // four different bytes
            b[k] = static_cast<uint8_t>(rng() & 0xFF);
            bool fresh = true;
            for (int j = 0; j < k; ++j) fresh = fresh && b[j] != b[k];
            if (fresh) ++k;
        }
        if (!stage_tables_right(b)) ++wrong;
        ++(stage_tables(b).ok ? ok : not_ok);
    }
    CHECK(wrong == 0);
    CHECK(ok > 1000 && not_ok > 1000);   // (both outcomes are common among random subsets)
}

int main(int argc, char **argv) {
    check_rows(argc, argv);
    check_budget_and_layout();
    check_space();
    check_trimming();
    check_records();
    check_small_rules();
    check_bucket_shift();
    check_uniform();
    check_phi_geometry();
    check_stage_tables();
    if (g_failed) return 1;
    std::printf("load_plan ok rows %d checks %d\n", (argc - 1) / 6, g_checks);
    return 0;
}
