// docdir_check.cpp -- rbg_docdir.hpp on the CPU: the builder and the lookup the device shares, against a plain count of the starts below q
// (DocList::doc_and_offset_at, doclist.hpp:46-50, over doc_bounds_rank, :77-79; size = the LAST start given + 1, :66).  Built with ASan + UBSan by
// tests/test_docdir_host.py, which asserts the printed number of lookups per path.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../rowbowt_amd/csrc/rbg_docdir.hpp"

using namespace rbg;

namespace {
unsigned long long g_path[kDocPathN] = {0, 0, 0};
unsigned long long g_tables = 0;
const uint64_t MAXU = ~uint64_t(0);

[[noreturn]] void fail(const char *what, uint64_t a, uint64_t b, uint64_t c) {
    std::printf("FAIL %s: %llu %llu %llu\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
    std::exit(1);
}

struct Table {
    std::vector<uint64_t> given, own_sorted;
    DocDir D;
    mutable uint64_t nchecks = 0;
    explicit Table(std::vector<uint64_t> g) : given(std::move(g)), own_sorted(given) {
        std::sort(own_sorted.begin(), own_sorted.end());
        if (!doc_dir_build(given.data(), given.size(), D)) fail("build", given.size(), 0, 0);
        const uint64_t nd = given.size();
        if (D.size != given.back() + 1) fail("size", D.size, given.back(), 0);
        // the shift rule: the directory is bounded, and no smaller shift would have been
        const uint64_t nb = (D.size >> D.shift) + 1;
        if (nb > uint64_t(kDocDirPerDoc) * nd || D.dir.size() != nb + 1) fail("directory size", nb, nd, D.dir.size());
        if (D.shift && (D.size >> (D.shift - 1)) < uint64_t(kDocDirPerDoc) * nd) fail("shift not minimal", D.shift, D.size, nd);
        for (size_t k = 0; k + 1 < D.dir.size(); ++k)
            if (D.dir[k] > D.dir[k + 1] || D.dir[k + 1] > nd) fail("directory order", k, D.dir[k], D.dir[k + 1]);
        ++g_tables;
    }
    // the rule, plainly: a count over the starts as given.  A table of more than 4096 documents takes the count at every 64th lookup and this file's own
    // sorted copy (std::lower_bound) at the others -- 2^16 starts times 2 * 10^5 positions is too much for a test
    uint32_t want_rank(uint64_t l) const {
        const uint64_t l1 = l + 1;   // wraps
        const uint64_t q = l1 > D.size ? D.size : l1;
        const uint32_t lb = static_cast<uint32_t>(std::lower_bound(own_sorted.begin(), own_sorted.end(), q) - own_sorted.begin());
        if (given.size() > 4096 && nchecks++ % 64 != 0) return lb;
        uint32_t j = 0;
        for (uint64_t s : given) j += s < q ? 1u : 0u;
        if (j != lb) fail("the check's own two counts", l, j, lb);
        return j;
    }
    void check(uint64_t l) const {
        const uint32_t want = want_rank(l);
        const uint32_t got = doc_rank(D.sorted.data(), D.dir.data(), D.size, D.shift, l, g_path);
        if (got != want) fail("rank", l, got, want);
        if (doc_rank_search(D.sorted.data(), D.sorted.size(), D.size, l) != want) fail("rank without the directory", l, want, 0);
        uint64_t off = 0;
        const uint32_t d = doc_and_offset(D.sorted.data(), D.dir.data(), D.size, D.shift, l, &off);
        if (want == 0 ? (d != kDocNone || off != l) : (d != want - 1 || off != l - D.sorted[want - 1])) fail("doc/offset", l, d, off);
    }
    void check_edges() const {
        for (uint64_t s : given) { check(s); check(s - 1); check(s + 1); }
        check(0); check(D.size - 2); check(D.size - 1); check(D.size); check(MAXU); check(MAXU - 1); check(D.size + 1);
    }
    void check_every(uint64_t upto) const { for (uint64_t l = 0; l <= upto; ++l) check(l); }
};

std::vector<uint64_t> equal_lengths(uint64_t nd, uint64_t len, uint64_t first = 0) {
    std::vector<uint64_t> s(nd);
    for (uint64_t j = 0; j < nd; ++j) s[j] = first + j * len;
    return s;
}
// one document holds 99 % of the text: the others crowd into the last buckets
std::vector<uint64_t> one_huge(uint64_t nd, uint64_t text) {
    std::vector<uint64_t> s(nd);
    s[0] = 0;
    const uint64_t rest = text / 100;
    for (uint64_t j = 1; j < nd; ++j) s[j] = text - rest + (j - 1) * (rest / nd);
    return s;
}
}  // namespace

int main() {
    // small tables, every position (and some beyond the size)
    for (uint64_t nd : {1u, 2u, 64u, 65u}) {
        Table t(equal_lengths(nd, 37));
        t.check_every(t.D.size + 70);
        t.check_edges();
        Table u(equal_lengths(nd, 1));     // documents of one symbol: every bucket has a start
        u.check_every(u.D.size + 5);
        u.check_edges();
        Table v(equal_lengths(nd, 37, 11));   // a first start above 0: positions before it have no document
        v.check_every(v.D.size + 5);
        v.check_edges();
    }
    // large tables: each start, start - 1, start + 1, and the ends
    for (uint64_t nd : {4096u, 65536u}) {
        Table(equal_lengths(nd, 100003)).check_edges();
        Table(equal_lengths(nd, 100003, 999)).check_edges();
        Table(one_huge(nd, uint64_t(3) * 1000 * 1000 * 1000)).check_edges();
    }
    Table(one_huge(64, 1000000)).check_every(1000100);
    Table(one_huge(65, 5000)).check_every(5100);
    // starts of 10 to 12 decimal digits, up to 3e11
    {
        std::vector<uint64_t> s;
        for (uint64_t j = 0; j < 520; ++j) s.push_back(uint64_t(1000000000) + j * uint64_t(574000000));
        s.push_back(uint64_t(300000000000));
        Table t(s);
        t.check_edges();
        std::mt19937_64 rng(7);
        for (int k = 0; k < 20000; ++k) t.check(rng() % (t.D.size + 1000));
    }
    // starts out of order: the last given start smallest, in the middle, second largest (size = the LAST given + 1, not the largest)
    {
        const std::vector<uint64_t> asc = equal_lengths(9, 50, 10);   // 10, 60, ..., 410
        for (size_t pick : {size_t(0), size_t(4), size_t(7)}) {
            std::vector<uint64_t> s;
            for (size_t j = asc.size(); j-- > 0;)
                if (j != pick) s.push_back(asc[j]);
            s.push_back(asc[pick]);
            Table t(s);
            if (t.D.size != asc[pick] + 1) fail("size of an out-of-order table", t.D.size, asc[pick], 0);
            t.check_every(500);
            t.check_edges();
        }
        // equal starts, and a last start of 2^64 - 1 (the size wraps to 0: nothing has a document)
        Table dup({5, 5, 5, 9, 9, 20});
        dup.check_every(40);
        Table wrap({3, 100, MAXU});
        wrap.check_every(200);
        wrap.check_edges();
        Table top({0, uint64_t(1) << 63, MAXU - 1});
        top.check_edges();
        top.check(uint64_t(1) << 63); top.check((uint64_t(1) << 63) - 1); top.check(MAXU - 2);
    }
    // random tables, a fixed seed: sizes 1..300, text lengths from tens to 2^40, equal / skewed / shuffled
    std::mt19937_64 rng(20240611);
    for (int it = 0; it < 4000; ++it) {
        const uint64_t nd = 1 + rng() % 300;
        const uint64_t text = uint64_t(10) + (rng() % (uint64_t(1) << (4 + rng() % 37)));
        std::vector<uint64_t> s(nd);
        const int kind = it % 4;
        for (uint64_t j = 0; j < nd; ++j) {
            if (kind == 0) s[j] = j * (text / nd + 1);
            else if (kind == 1) s[j] = rng() % text;
            else if (kind == 2) s[j] = j == 0 ? 0 : text - 1 - (rng() % (text / 50 + 1));   // crowded at the end
            else s[j] = (rng() % 8 == 0) ? rng() % text : (text / 2 + rng() % 16);           // crowded in the middle
        }
        if (kind != 0 || it % 8 == 0)
            for (uint64_t j = nd; j > 1; --j) std::swap(s[j - 1], s[rng() % j]);
        Table t(s);
        t.check_edges();
        for (int k = 0; k < 40; ++k) t.check(rng() % (text + 5));
        if (text < 400) t.check_every(text + 3);
    }
    // refusals of the builder
    {
        DocDir D;
        std::vector<uint64_t> s(kDocMaxDocs + 1, 1);
        if (doc_dir_build(s.data(), 0, D) || doc_dir_build(s.data(), kDocMaxDocs + 1, D) || !doc_dir_build(s.data(), kDocMaxDocs, D)) fail("builder limits", 0, 0, 0);
    }
    std::printf("docdir ok tables %llu directory %llu scan %llu search %llu\n", g_tables, g_path[kDocPathDir], g_path[kDocPathScan], g_path[kDocPathSearch]);
    return 0;
}
