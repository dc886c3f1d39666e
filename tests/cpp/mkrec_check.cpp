// CPU test of the marker directory (rowbowt_amd/csrc/rbg_mkdir.hpp): the shift rule, the gates, the directory and bucket-record builder that
// upload_marker_table runs, and the arithmetic with which marker_query answers -- at the bucket widths, row offsets, value counts and value
// offsets that no index of test size reaches.  Every table is built with the real builder; every query (lo <= hi) is answered
//   - through the records (mk_rec_answer; a bucket that overflows its record hands over to marker_span_arrays from the records' first runs),
//   - through the directory and the run arrays (marker_span_arrays from the two bucket entries),
//   - by binary search over the run ends and starts,
// and each answer {first run, one past the last run, first value, number of values} is compared with a scan over all runs
// (start <= hi && end >= lo).  Only the offsets of the values are needed, never the values, so offsets of 2^32 and more cost nothing.
// The control flow around the shared functions (rows beyond n, the two bucket numbers, lo and hi relative to their buckets) is restated here
// from marker_query (rbg_device.hpp), which keeps the loads.  The first mismatch ends the run.
// Prints "mkrec ok records <a> overflow <b> directory <c> bsearch <d>": the comparisons made per path.
#include <cinttypes>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "../../rowbowt_amd/csrc/rbg_mkdir.hpp"

namespace {

using rbg::MkRec;
using rbg::MkView;

struct Table {
    uint64_t n = 0;
    std::vector<uint64_t> start, end, off;   // off: one more entry than runs, ascending, from any base
    void add(uint64_t s, uint64_t e, uint64_t cnt) {
        if (off.empty()) off.push_back(0);
        start.push_back(s); end.push_back(e); off.push_back(off.back() + cnt);
    }
    void rebase(uint64_t base) { for (uint64_t &o : off) o += base; }
    uint64_t nruns() const { return start.size(); }
};
struct Built {
    uint32_t shift = 0;
    bool has_rec = false;
    std::vector<uint32_t> bucket;
    std::vector<MkRec> recs;
};
struct Ans {
    bool any = false;
    uint64_t f = 0, l = 0, src = 0, cnt = 0;
    bool operator==(const Ans &o) const { return any == o.any && (!any || (f == o.f && l == o.l && src == o.src && cnt == o.cnt)); }
};

uint64_t g_rec = 0, g_over = 0, g_dir = 0, g_bin = 0;
// what the cases are there to reach, counted on the way
uint64_t g_over_lo_only = 0, g_over_hi_only = 0, g_over_both = 0, g_lo_rel_max = 0, g_hi_rel_max = 0, g_clamped = 0, g_cnt_max = 0, g_off_cross = 0;

Built build(const Table &t, uint32_t shift) {
    Built b;
    b.shift = shift;
    rbg::mk_build_dir(t.end.data(), t.nruns(), t.n, shift, b.bucket);
    b.has_rec = rbg::mk_rec_shift_ok(shift) && rbg::mk_rec_vals_ok(t.off.back());
    if (b.has_rec) rbg::mk_build_recs(t.start.data(), t.end.data(), t.off.data(), t.nruns(), t.off.back(), shift, b.bucket, b.recs);
    return b;
}
MkView view(const Table &t, const Built &b) {
    return MkView{t.start.data(), t.end.data(), t.off.data(), nullptr, t.nruns(), t.n, b.bucket.data(), b.has_rec ? b.recs.data() : nullptr, b.shift};
}

Ans scan(const Table &t, uint64_t lo, uint64_t hi) {
    Ans a;
    if (lo >= t.n) return a;
    for (uint64_t j = 0; j < t.nruns(); ++j)
        if (t.start[j] <= hi && t.end[j] >= lo) {
            if (!a.any) { a.any = true; a.f = j; }
            a.l = j + 1;
        }
    if (a.any) { a.src = t.off[a.f]; a.cnt = t.off[a.l] - a.src; }
    return a;
}
Ans from_span(const Table &t, uint64_t f, uint64_t l) {
    Ans a;
    if (l <= f) return a;
    a.any = true; a.f = f; a.l = l; a.src = t.off[f]; a.cnt = t.off[l] - a.src;
    return a;
}
Ans by_records(const Table &t, const Built &b, uint64_t lo, uint64_t hi, bool *overflowed) {
    *overflowed = false;
    if (lo >= t.n) return Ans();
    if (hi >= t.n) hi = t.n - 1;
    const uint32_t sh = b.shift;
    const uint64_t b0 = lo >> sh, b1 = hi >> sh;
    const MkRec R0 = b.recs.at(b0), R1 = b.recs.at(b1);
    const uint32_t lo_rel = static_cast<uint32_t>(lo - (b0 << sh)), hi_rel = static_cast<uint32_t>(hi - (b1 << sh));
    const bool o0 = R0.nin == rbg::kMkRecOverflow, o1 = R1.nin == rbg::kMkRecOverflow;
    if (b0 != b1) { g_over_lo_only += o0 && !o1; g_over_hi_only += !o0 && o1; g_over_both += o0 && o1; }
    uint64_t f, l, off_f, off_l;
    if (!o0 && !o1) {
        rbg::mk_rec_answer(R0, R1, lo_rel, hi_rel, &f, &l, &off_f, &off_l);
        g_lo_rel_max += lo_rel == 0xFFFF; g_hi_rel_max += hi_rel == 0xFFFF;
        for (uint32_t j = 0; j < R0.nin; ++j) {
            g_clamped += R0.e_off[j] == 0xFFFF && t.end[R0.a + j] - (b0 << sh) > 0xFFFF;
            g_cnt_max += R0.cnt[j] == 0xFFFF;
        }
        g_off_cross += (off_f >> 32) != R0.off_hi || (off_l >> 32) != R1.off_hi;
        Ans a;
        if (l <= f) return a;
        a.any = true; a.f = f; a.l = l; a.src = off_f; a.cnt = off_l - off_f;
        return a;
    }
    *overflowed = true;
    const MkView v = view(t, b);
    rbg::marker_span_arrays(v, lo, hi, R0.a, R1.a, &f, &l, nullptr);
    return from_span(t, f, l);
}
Ans by_directory(const Table &t, const Built &b, uint64_t lo, uint64_t hi) {
    if (lo >= t.n) return Ans();
    if (hi >= t.n) hi = t.n - 1;
    const MkView v = view(t, b);
    uint64_t f, l;
    rbg::marker_span_arrays(v, lo, hi, b.bucket.at(lo >> b.shift), b.bucket.at(hi >> b.shift), &f, &l, nullptr);
    return from_span(t, f, l);
}
Ans by_bsearch(const Table &t, uint64_t lo, uint64_t hi) {
    if (lo >= t.n) return Ans();
    if (hi >= t.n) hi = t.n - 1;
    uint64_t a = 0, z = t.nruns();
    while (a < z) { const uint64_t m = a + ((z - a) >> 1); if (t.end[m] < lo) a = m + 1; else z = m; }
    const uint64_t f = a;
    a = 0; z = t.nruns();
    while (a < z) { const uint64_t m = a + ((z - a) >> 1); if (t.start[m] <= hi) a = m + 1; else z = m; }
    return from_span(t, f, a);
}

bool fail(const char *path, const char *what, const Table &t, uint32_t shift, uint64_t lo, uint64_t hi, const Ans &got, const Ans &want) {
    std::fprintf(stderr, "%s, %s: shift %u n %" PRIu64 " runs %" PRIu64 " [%" PRIu64 ", %" PRIu64 "]: got %d {%" PRIu64 ", %" PRIu64 ", %" PRIu64 ", %" PRIu64
                 "}, want %d {%" PRIu64 ", %" PRIu64 ", %" PRIu64 ", %" PRIu64 "}\n", what, path, shift, t.n, t.nruns(), lo, hi, got.any ? 1 : 0, got.f, got.l,
                 got.src, got.cnt, want.any ? 1 : 0, want.f, want.l, want.src, want.cnt);
    return false;
}
bool query(const char *what, const Table &t, const Built &b, uint64_t lo, uint64_t hi) {
    const Ans want = scan(t, lo, hi);
    if (b.has_rec) {
        bool over;
        const Ans got = by_records(t, b, lo, hi, &over);
        if (!(got == want)) return fail(over ? "records, overflow to the arrays" : "records", what, t, b.shift, lo, hi, got, want);
        ++(over ? g_over : g_rec);
    }
    Ans got = by_directory(t, b, lo, hi);
    if (!(got == want)) return fail("directory", what, t, b.shift, lo, hi, got, want);
    ++g_dir;
    got = by_bsearch(t, lo, hi);
    if (!(got == want)) return fail("bsearch", what, t, b.shift, lo, hi, got, want);
    ++g_bin;
    return true;
}

// the rows worth asking about: every run's start and end and their neighbours, both ends of every bucket, n - 1, n, n + 5
std::vector<uint64_t> edge_rows(const Table &t, uint32_t shift) {
    std::set<uint64_t> p = {0, t.n - 1, t.n, t.n + 5};
    for (uint64_t j = 0; j < t.nruns(); ++j)
        for (uint64_t x : {t.start[j], t.end[j]}) { if (x) p.insert(x - 1); p.insert(x); p.insert(x + 1); }
    for (uint64_t b = 0; b <= (t.n >> shift); ++b) { p.insert(b << shift); p.insert(((b + 1) << shift) - 1); }
    return std::vector<uint64_t>(p.begin(), p.end());
}
bool all_pairs(const char *what, const Table &t, uint32_t shift) {
    for (uint64_t j = 0; j < t.nruns(); ++j)   // what the library checks before it takes a table (markers_valid), and the text table's bound
        if (t.end[j] < t.start[j] || (j && t.start[j] <= t.end[j - 1]) || t.end[j] >= t.n) { std::fprintf(stderr, "%s: run %" PRIu64 " is not a table's\n", what, j); return false; }
    const Built b = build(t, shift);
    if (b.has_rec != (shift <= 16)) { std::fprintf(stderr, "%s: records at shift %u, or none below?\n", what, shift); return false; }   // (every all_pairs table has fewer than 2^40 values)
    const std::vector<uint64_t> p = edge_rows(t, shift);
    for (size_t i = 0; i < p.size(); ++i)
        for (size_t k = i; k < p.size(); ++k)
            if (!query(what, t, b, p[i], p[k])) return false;
    return true;
}

uint64_t pick(std::mt19937_64 &rng, std::initializer_list<uint64_t> of) { return of.begin()[rng() % of.size()]; }

// runs and gaps of one row, a few rows, a bucket less one, a bucket, a bucket and one, several buckets; values per run from none to more than a record counts
Table random_table(std::mt19937_64 &rng, uint32_t shift, uint64_t max_runs, bool small_counts) {
    const uint64_t W = uint64_t(1) << shift;
    Table t;
    t.n = (1 + rng() % 8) * W - rng() % W;
    uint64_t pos = pick(rng, {0, 0, 1, W / 2, W - 1, W});
    while (pos < t.n && t.nruns() < max_runs) {
        const uint64_t len = std::max<uint64_t>(1, pick(rng, {1, 1, 2, 3, W / 3, W - 1, W, W + 1, 2 * W + 3, 3 * W}));
        const uint64_t e = std::min(pos + len - 1, t.n - 1);
        const uint64_t cnt = small_counts || rng() % 16 ? pick(rng, {0, 1, 1, 1, 2, 2, 5, 9}) : pick(rng, {65534, 65535, 65535, 65536, 65536, 65537, 70000, 200000});
        t.add(pos, e, cnt);
        pos = e + pick(rng, {1, 1, 1, 2, 3, W / 2 + 1, W, 2 * W});
    }
    if (t.off.empty()) t.off.push_back(0);
    const uint64_t total = t.off.back(), top = (uint64_t(1) << 40) - 1;
    t.rebase(pick(rng, {0, 0, 7, (uint64_t(1) << 32) - 3, (uint64_t(1) << 32) - 65536, (uint64_t(1) << 32) + 1, (uint64_t(1) << 39) - 2, top - total}));
    return t;
}

bool expect(bool ok, const char *what) {
    if (!ok) std::fprintf(stderr, "%s\n", what);
    return ok;
}

bool gates_and_shift_rule() {
    bool ok = true;
    // ---- the gates
    for (uint32_t s = 0; s <= 20; ++s) ok = ok && expect(rbg::mk_rec_shift_ok(s) == (s <= 16), "the shift gate: records up to 2^16 rows a bucket");
    ok = ok && expect(rbg::mk_rec_vals_ok((uint64_t(1) << 40) - 1) && !rbg::mk_rec_vals_ok(uint64_t(1) << 40) && rbg::mk_rec_vals_ok(0), "the value gate: 2^40 - 1 / 2^40");
    ok = ok && expect(rbg::mk_rec_switch_on(nullptr) && rbg::mk_rec_switch_on("") && rbg::mk_rec_switch_on("1") && rbg::mk_rec_switch_on("10") &&
                      !rbg::mk_rec_switch_on("0") && !rbg::mk_rec_switch_on("01"), "the RBG_MK_REC switch");
    const uint64_t GiB = uint64_t(1) << 30;
    // an eighth of the free bytes binds below 128 GiB free: 64 GiB free -> 8 GiB of records = 2^28 buckets
    ok = ok && expect(rbg::mk_rec_fits(uint64_t(1) << 28, 64 * GiB) && !rbg::mk_rec_fits((uint64_t(1) << 28) + 1, 64 * GiB), "rec_fits: the bucket where it flips at 64 GiB free");
    ok = ok && expect(rbg::mk_rec_fits(1000, 1000 * 32 * 8) && !rbg::mk_rec_fits(1000, 1000 * 32 * 8 - 1), "rec_fits: the byte where it flips, 1000 buckets");
    // the 16 GiB cap binds above: 2^29 buckets whatever is free
    for (uint64_t free_b : {128 * GiB, 128 * GiB + 256, 200 * GiB, 288 * GiB})
        ok = ok && expect(rbg::mk_rec_fits(uint64_t(1) << 29, free_b) && !rbg::mk_rec_fits((uint64_t(1) << 29) + 1, free_b), "rec_fits: the bucket where it flips under the cap");
    ok = ok && expect(!rbg::mk_rec_fits(uint64_t(1) << 29, 128 * GiB - 8) && rbg::mk_rec_fits(0, 0) && !rbg::mk_rec_fits(1, 255) && rbg::mk_rec_fits(1, 256), "rec_fits: just below the cap; nothing free");
    ok = ok && expect(rbg::mk_rec_wanted(16, nullptr, 5, 100, GiB) && !rbg::mk_rec_wanted(17, nullptr, 5, 100, GiB) && !rbg::mk_rec_wanted(16, "0", 5, 100, GiB) &&
                      !rbg::mk_rec_wanted(16, nullptr, uint64_t(1) << 40, 100, GiB) && !rbg::mk_rec_wanted(16, nullptr, 5, 100, 100 * 32 * 8 - 1), "every gate closes the records alone");
    // ---- the shift rule: the least shift <= 20 with (n >> shift) <= 2 nruns, on both sides of both thresholds of the shifts 14..20
    for (uint32_t s = 14; s <= 20; ++s)
        for (uint64_t r : {uint64_t(1), uint64_t(3), uint64_t(100), uint64_t(8000), uint64_t(1) << 31}) {
            const uint64_t first = (2 * r + 1) << (s - 1), last = ((2 * r + 1) << s) - 1;   // the least and the greatest n of shift s
            ok = ok && expect(rbg::mk_dir_shift(first, r) == s && rbg::mk_dir_shift(first - 1, r) == s - 1 && rbg::mk_dir_shift(last, r) == s &&
                              rbg::mk_dir_shift(last + 1, r) == (s < 20 ? s + 1 : 20), "the shift rule at a threshold");
        }
    ok = ok && expect(rbg::mk_dir_shift(~uint64_t(0), 1) == 20 && rbg::mk_dir_shift(uint64_t(1) << 40, 0) == 20 && rbg::mk_dir_shift(0, 0) == 0 && rbg::mk_dir_shift(1, 1) == 0, "the cap at 20; no rows");
    // the tables of tests/test_gpu_marker_dir.py: (n, nruns) -> the shift it means to reach
    const uint64_t gpu_n = 8401260;
    const struct { uint64_t nruns; uint32_t shift; } gpu[] = {{200, 15}, {100, 16}, {64, 16}, {127, 16}, {128, 15}, {63, 17}, {40, 17}, {32, 17}, {31, 18}, {7, 20}, {4, 20}, {3, 20}};
    for (const auto &g : gpu) ok = ok && expect(rbg::mk_dir_shift(gpu_n, g.nruns) == g.shift, "the shift of a GPU test table");
    ok = ok && expect(rbg::mk_dir_buckets(gpu_n, 16) == 130 && rbg::mk_dir_buckets(gpu_n, 20) == 10, "buckets: two more than whole ones");
    return ok;
}

// shift 16: the row offsets and value counts at the ends of what a record holds
Table edges16() {
    const uint64_t W = 0x10000;
    Table t;
    t.n = 25 * W + 1234;
    t.add(5, 5, 1);
    t.add(W - 10, W, 2);                           // starts before F = W, ends on F
    t.add(W + 1, W + 3, 1);                        // starts on F + 1
    t.add(2 * W, 2 * W + 5, 3);                    // starts on F; bucket 2 lists three runs
    t.add(2 * W + 100, 2 * W + 0xFFFE, 1);         // ends on F + 0xFFFE
    t.add(2 * W + 0xFFFF, 2 * W + 0xFFFF, 2);      // starts and ends on F + 0xFFFF
    t.add(4 * W + 9, 4 * W + 0xFFFF, 1);           // ends on F + 0xFFFF; bucket 4 lists one run
    t.add(6 * W + 7, 6 * W + 0x10000, 4);          // ends on F + 0x10000: clamped
    t.add(8 * W + 50, 8 * W + 0x2FFFF, 2);         // ends on F + 0x2FFFF; bucket 11 lists no run
    t.add(12 * W, 15 * W - 1, 3);                  // covers the buckets 12, 13, 14 and nothing else
    t.add(17 * W + 1, 17 * W + 1, 1);              // bucket 17 holds four runs: overflow
    t.add(17 * W + 3, 17 * W + 4, 2);
    t.add(17 * W + 10, 17 * W + 20, 1);
    t.add(17 * W + 0xFFF0, 17 * W + 0xFFFF, 1);
    t.add(19 * W + 5, 19 * W + 6, 0);              // no value
    t.add(19 * W + 0xFFFF, 20 * W + 2, 1);         // starts on F + 0xFFFF and goes on
    t.add(20 * W + 10, 20 * W + 20, 65535);        // as many values as a record counts
    t.add(22 * W + 1, 22 * W + 2, 1);
    t.add(22 * W + 100, 22 * W + 200, 65536);      // one more: overflow, between two small runs of the same bucket
    t.add(22 * W + 300, 22 * W + 301, 2);
    t.add(25 * W + 1000, 25 * W + 1233, 1);        // ends on n - 1
    return t;
}

}  // namespace

int main() {
    bool ok = gates_and_shift_rule();
    // ---- shift 16 by hand, from three value offsets: 0, across 2^32 inside bucket 2's listed runs, up to 2^40 - 1
    {
        Table t = edges16();
        ok = ok && all_pairs("edges at shift 16", t, 16);
        ok = ok && expect(g_over_lo_only && g_over_hi_only && g_over_both, "overflow on one side only and on both") &&
             expect(g_lo_rel_max >= 20 && g_hi_rel_max >= 20 && g_clamped >= 20, "lo, hi and run ends on a bucket's last row") &&
             expect(g_cnt_max && g_over, "runs of 65535 and of 65536 values");
        // the offset of bucket 2's record is 2^32 - 3 (four values precede it) and its runs hold 3, 1 and 2 values
        const uint64_t before = g_off_cross;
        Table u = t; u.rebase((uint64_t(1) << 32) - 7);
        ok = ok && expect(u.off[3] == (uint64_t(1) << 32) - 3, "the offset that crosses 2^32") && all_pairs("edges at shift 16, offsets across 2^32", u, 16);
        ok = ok && expect(g_off_cross > before, "value offsets that cross 2^32 inside a record's listed runs");
        Table v = t; v.rebase((uint64_t(1) << 40) - 1 - t.off.back());
        ok = ok && expect(v.off.back() == (uint64_t(1) << 40) - 1, "offsets up to 2^40 - 1") && all_pairs("edges at shift 16, offsets up to 2^40 - 1", v, 16);
        Table w = t; w.rebase((uint64_t(1) << 40) - t.off.back());   // one value more: no records
        ok = ok && expect(!build(w, 16).has_rec, "2^40 values: the directory answers");
        // the same runs under the neighbouring bucket widths, and where the directory answers alone
        for (uint32_t s : {14u, 15u, 17u, 20u}) ok = ok && all_pairs("the shift 16 edges at another shift", t, s);
    }
    // ---- forced shifts: tables laid out by the bucket width
    std::mt19937_64 rng(20240901);
    for (uint32_t s : {0u, 1u, 8u, 14u, 15u, 16u, 17u, 20u})
        for (int k = 0; k < 24 && ok; ++k) ok = all_pairs("forced shift", random_table(rng, s, 12, k % 2 == 0), s);
    const uint64_t forced_dir = g_dir;
    // ---- random tables, shifts 0..16
    for (int k = 0; k < 4000 && ok; ++k) {
        const uint32_t s = static_cast<uint32_t>(rng() % 17);
        const Table t = random_table(rng, s, 24, rng() % 3 == 0);
        const Built b = build(t, s);
        const std::vector<uint64_t> p = edge_rows(t, s);
        for (int q = 0; q < 60 && ok; ++q) {
            uint64_t lo, hi;
            if (q < 40) { lo = p[rng() % p.size()]; hi = p[rng() % p.size()]; }
            else { lo = rng() % (t.n + 3); hi = lo + pick(rng, {0, 1, 5, uint64_t(1) << s, (uint64_t(2) << s) + 1, rng() % (t.n + 1)}); }
            if (hi < lo) std::swap(lo, hi);
            ok = query("random table", t, b, lo, hi);
        }
    }
    ok = ok && expect(g_dir > forced_dir && g_dir == g_bin && g_rec + g_over < g_dir, "every path was taken");
    if (!ok) return 1;
    std::printf("mkrec ok records %" PRIu64 " overflow %" PRIu64 " directory %" PRIu64 " bsearch %" PRIu64 "\n", g_rec, g_over, g_dir, g_bin);
    return 0;
}
