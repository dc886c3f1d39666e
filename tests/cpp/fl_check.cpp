// The FL index that host and device share (rowbowt_amd/csrc/rbg_fl.hpp), on the host: fl_build and fl_step at every row against a select over the expanded BWT,
// on inputs that hold every shape the structure distinguishes (each asserted present); 8-byte positions over run arrays whose lengths carry rows across
// 2^32, against the arithmetic written out again over the runs; and rbg_sam.hpp's formatter with two extension records.  Stand-alone:
// g++ -fsanitize=address,undefined tests/cpp/fl_check.cpp.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../rowbowt_amd/csrc/rbg_fl.hpp"
#include "../../rowbowt_amd/csrc/rbg_sam.hpp"

using namespace rbg;

static unsigned long long g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

struct Runs {
    std::vector<uint8_t> heads;
    std::vector<uint64_t> start;    // R + 1
    uint64_t F[256];
};
static Runs runs_of(const std::vector<std::pair<uint8_t, uint64_t>> &rl) {
    Runs r;
    uint64_t n = 0, count[256] = {};
    for (const auto &p : rl) {
        CHECK(p.second > 0 && (r.heads.empty() || r.heads.back() != p.first));
        r.heads.push_back(p.first);
        r.start.push_back(n);
        n += p.second;
        count[p.first] += p.second;
    }
    r.start.push_back(n);
    uint64_t acc = 0;
    for (int c = 0; c < 256; ++c) { r.F[c] = acc; acc += count[c]; }
    return r;
}
static std::vector<std::pair<uint8_t, uint64_t>> rle(const std::string &bwt) {
    std::vector<std::pair<uint8_t, uint64_t>> rl;
    for (char ch : bwt) {
        const uint8_t c = static_cast<uint8_t>(ch);
        if (!rl.empty() && rl.back().first == c) rl.back().second += 1; else rl.push_back({c, 1});
    }
    return rl;
}

// what the shapes below must show at least once
struct Seen {
    unsigned single_run = 0, absent = 0, shift0 = 0, full_bucket = 0, run_over_buckets = 0, first_last = 0, terminator = 0, separator = 0, search = 0;
};

// the run of rank k by a scan: the arithmetic of the rule written out again
static uint64_t naive_fl(const Runs &r, uint8_t c, uint64_t k) {
    uint64_t seen = 0;
    for (size_t g = 0; g < r.heads.size(); ++g) {
        if (r.heads[g] != c) continue;
        const uint64_t len = r.start[g + 1] - r.start[g];
        if (k < seen + len) return r.start[g] + (k - seen);
        seen += len;
    }
    return kFlNone;
}

template <typename P>
static void check_shapes(const FlIndex &X, Seen &seen) {
    for (uint32_t j = 0; j < kFlBases; ++j) {
        seen.single_run += X.runs[j] == 1;
        seen.absent += X.runs[j] == 0;
        if (!X.runs[j]) { CHECK(X.total[j] == 0 && X.dir_entries[j] == 0); continue; }
        seen.shift0 += X.shift[j] == 0;
        CHECK((X.runs[j] << X.shift[j]) <= X.total[j] && (X.shift[j] == 63 || (X.runs[j] << (X.shift[j] + 1)) > X.total[j]));
        CHECK(X.dir_entries[j] == (X.total[j] >> X.shift[j]) + 2);
        const FlEnt<P> *ent = reinterpret_cast<const FlEnt<P> *>(X.blob.data() + X.ent_at[j]);
        const P *dir = reinterpret_cast<const P *>(X.blob.data() + X.dir_at[j]);
        CHECK(ent[X.runs[j]].cum == X.total[j] && ent[X.runs[j]].pos == X.n && ent[0].cum == 0);
        for (uint64_t b = 0; b + 1 < X.dir_entries[j]; ++b) {
            CHECK(dir[b] <= dir[b + 1] && dir[b + 1] <= X.runs[j] && dir[b + 1] - dir[b] <= (uint64_t(1) << X.shift[j]));   // a bounded search, never the whole list
            if ((b << X.shift[j]) < X.total[j]) CHECK(ent[dir[b]].cum <= (b << X.shift[j]) && ent[dir[b] + 1].cum > (b << X.shift[j]));
            else CHECK(dir[b] == X.runs[j]);
            if (X.shift[j] > 0 && dir[b + 1] - dir[b] == (uint64_t(1) << X.shift[j])) {
                bool ones = true;
                for (uint64_t g = dir[b]; g < dir[b + 1]; ++g) ones = ones && ent[g + 1].cum - ent[g].cum == 1;
                seen.full_bucket += ones;
            }
            seen.run_over_buckets += b + 2 < X.dir_entries[j] && dir[b] == dir[b + 1] && dir[b + 1] == dir[b + 2] && ((b + 2) << X.shift[j]) < X.total[j];
        }
    }
    CHECK(X.bytes() == fl_base_bytes(X.total[0], X.runs[0], X.pos_bytes) + fl_base_bytes(X.total[1], X.runs[1], X.pos_bytes) +
                           fl_base_bytes(X.total[2], X.runs[2], X.pos_bytes) + fl_base_bytes(X.total[3], X.runs[3], X.pos_bytes));
}

// every row of a BWT given as a string, at both widths, against select over the expanded BWT
static void check_text(const std::string &bwt, Seen &seen) {
    const Runs r = runs_of(rle(bwt));
    const uint64_t n = bwt.size();
    for (uint32_t pb : {4u, 8u}) {
        FlIndex X;
        CHECK(fl_build(r.heads.data(), r.start.data(), r.heads.size(), r.F, pb, X));
        CHECK(X.n == n && X.pos_bytes == pb);
        if (pb == 4) check_shapes<uint32_t>(X, seen); else check_shapes<uint64_t>(X, seen);
        const FlView v = X.view(X.blob.data());
        // F order: the symbols ascending, the k-th occurrence of c in the BWT at row F[c] + k
        std::vector<std::vector<uint64_t>> occ(256);
        for (uint64_t i = 0; i < n; ++i) occ[static_cast<uint8_t>(bwt[i])].push_back(i);
        uint64_t row = 0;
        for (int c = 0; c < 256; ++c)
            for (size_t k = 0; k < occ[c].size(); ++k, ++row) {
                unsigned long long probes = 0;
                const FlStep st = pb == 4 ? fl_step<uint32_t>(v, row, &probes) : fl_step<uint64_t>(v, row, &probes);
                const bool base = c == 'A' || c == 'C' || c == 'G' || c == 'T';
                if (base) {
                    CHECK(st.sym == static_cast<uint32_t>(c) && st.next == occ[c][k]);
                    seen.first_last += k == 0 || k + 1 == occ[c].size();
                    seen.search += probes > 0;
                } else {
                    CHECK(st.sym == 0 && st.next == kFlNone);
                    seen.terminator += c == 1;
                    seen.separator += c == '$';
                }
            }
        CHECK(row == n);
    }
}

// few runs of huge lengths at 8-byte positions: rows on both sides of 2^32, no expansion
static void check_huge() {
    const uint64_t G = uint64_t(1) << 30;
    const Runs r = runs_of({{'C', 3 * G + 5}, {1, 1}, {'A', 2 * G + 1}, {'C', 7}, {'T', 5 * G}, {'A', 3}, {'G', 1}, {'T', G + 11}, {'C', 2 * G}, {'N', 9}, {'A', 3 * G}});
    FlIndex X;
    CHECK(!fl_build(r.heads.data(), r.start.data(), r.heads.size(), r.F, 4, X));    // n >= 2^32 does not fit 4-byte positions
    CHECK(fl_build(r.heads.data(), r.start.data(), r.heads.size(), r.F, 8, X));
    Seen s;
    check_shapes<uint64_t>(X, s);
    const FlView v = X.view(X.blob.data());
    const uint64_t n = X.n, two32 = uint64_t(1) << 32;
    CHECK(n > 4 * two32);
    std::vector<uint64_t> rows = {0, 1, n - 1};
    for (uint64_t mult = 1; mult <= 4; ++mult)
        for (int d = -3; d <= 3; ++d) rows.push_back(mult * two32 + d);
    for (uint32_t j = 0; j < kFlBases; ++j) {
        const uint64_t f = r.F[fl_base_byte(j)];
        for (uint64_t k : {uint64_t(0), uint64_t(1), X.total[j] / 2, X.total[j] - 2, X.total[j] - 1}) rows.push_back(f + k);
        for (uint64_t g = 0; g + 1 < X.dir_entries[j]; g += 1 + X.dir_entries[j] / 50) {
            const uint64_t k = g << X.shift[j];
            if (k < X.total[j]) { rows.push_back(f + k); if (k) rows.push_back(f + k - 1); }
        }
    }
    unsigned crossed = 0;
    for (uint64_t row : rows) {
        uint8_t c = 0;
        for (int b = 255; b >= 0; --b)
            if (r.F[b] <= row) { c = static_cast<uint8_t>(b); break; }
        // (F[c] <= row and c is the largest such byte that occurs: skip bytes that do not occur)
        while (c > 0 && r.F[c] == (c == 255 ? n : r.F[c + 1]) ) --c;
        const FlStep st = fl_step<uint64_t>(v, row);
        if (c == 'A' || c == 'C' || c == 'G' || c == 'T') {
            const uint64_t want = naive_fl(r, c, row - r.F[c]);
            CHECK(st.sym == c && st.next == want);
            crossed += (row < two32) != (want < two32) || row >= two32;
        } else {
            CHECK(st.sym == 0 && st.next == kFlNone);
        }
    }
    CHECK(crossed > 20);
}

// the formatter with two records: the length equals the bytes written, MD starts and ends with a number and re-expands to both flanks
static void check_lines() {
    const std::string name = "read/1", rname = "hapX";
    unsigned long long seed = 99;
    auto rnd = [&](unsigned mod) { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return static_cast<unsigned>((seed >> 33) % mod); };
    unsigned both_moved = 0, clip_gone = 0;
    for (int it = 0; it < 3000; ++it) {
        const uint64_t a = rnd(40), seed_len = 20 + rnd(100), tail = rnd(40), m = a + seed_len + tail, b = a + seed_len;
        SamExtend x, y;
        std::memset(&x, 0, sizeof x);
        std::memset(&y, 0, sizeof y);
        auto fill = [&](SamExtend &z, uint64_t room) {
            z.ext = static_cast<uint32_t>(room ? rnd(static_cast<unsigned>(room) + 1) : 0);
            const uint32_t want = z.ext > 1 ? rnd(5) : 0;
            uint32_t at = 0;
            for (uint32_t k = 0; k < want && at + 1 < z.ext; ++k) {      // ascending t, never the last extended base (an extension ends on a match)
                const uint32_t t = at + rnd(z.ext - 1 - at);
                z.mis_t[z.nm] = t;
                z.mis_ref[z.nm] = static_cast<uint8_t>("ACGT"[rnd(4)]);
                z.nm += 1;
                at = t + 1;
            }
            z.score = static_cast<int32_t>(z.ext) - 5 * static_cast<int32_t>(z.nm);
            if (z.score < 0) { z.nm = 0; z.score = static_cast<int32_t>(z.ext); std::memset(z.mis_t, 0, sizeof z.mis_t); std::memset(z.mis_ref, 0, sizeof z.mis_ref); }
        };
        fill(x, a);
        fill(y, tail);
        both_moved += x.ext > 0 && y.ext > 0;
        clip_gone += tail > 0 && y.ext == tail;
        for (int hit = 1; hit <= 2; ++hit)
            for (int rev = 0; rev < 2; ++rev) {
                SamLine L{name.size(), true, rev != 0, static_cast<uint64_t>(hit), 3, rname.size(), 1000 + x.ext, m, a, b, true};
                std::string seq(m, 'C'), qual(m, 'I');
                for (uint64_t j = 0; j < m; ++j) seq[j] = "ACGT"[(j * 5 + a) % 4];
                const uint64_t n = sam_line_len(L, &x, &y);
                std::vector<char> buf(n + 32, '#');
                sam_put_line(buf.data() + 16, L, name.data(), rname.data(), seq.data(), qual.data(), &x, &y);
                for (int j = 0; j < 16; ++j) CHECK(buf[j] == '#' && buf[16 + n + j] == '#');
                CHECK(buf[16 + n - 1] == '\n');
                const std::string line(buf.data() + 16, n);
                CHECK(line.find('#') == std::string::npos);
                // the fields
                std::vector<std::string> f;
                size_t p = 0;
                for (;;) { const size_t q = line.find('\t', p); f.push_back(line.substr(p, q == std::string::npos ? n - 1 - p : q - p)); if (q == std::string::npos) break; p = q + 1; }
                CHECK(f.size() == 16);
                std::string cig;
                if (a - x.ext) cig += std::to_string(a - x.ext) + "S";
                cig += std::to_string(seed_len + x.ext + y.ext) + "M";
                if (tail - y.ext) cig += std::to_string(tail - y.ext) + "S";
                CHECK(f[5] == cig && f[3] == "1000");
                CHECK(f[13] == "NM:i:" + std::to_string(x.nm + y.nm) && f[15] == "AS:i:" + std::to_string(seed_len + x.score + y.score));
                const std::string md = f[14].substr(5);
                CHECK(f[14].compare(0, 5, "MD:Z:") == 0 && !md.empty() && md.front() >= '0' && md.front() <= '9' && md.back() >= '0' && md.back() <= '9');
                // MD re-expanded: the mismatch positions within [a - eL, b + eR) and their bases
                std::vector<std::pair<uint64_t, char>> want, got;
                for (uint32_t i = x.nm; i-- > 0;) want.push_back({x.ext - 1 - x.mis_t[i], static_cast<char>(x.mis_ref[i])});
                for (uint32_t i = 0; i < y.nm; ++i) want.push_back({x.ext + seed_len + y.mis_t[i], static_cast<char>(y.mis_ref[i])});
                uint64_t at = 0, num = 0;
                bool digit_before = false;
                for (char ch : md) {
                    if (ch >= '0' && ch <= '9') { num = num * 10 + static_cast<uint64_t>(ch - '0'); digit_before = true; continue; }
                    CHECK(digit_before);                       // never two bases in a row without a number between them
                    at += num;
                    got.push_back({at, ch});
                    at += 1; num = 0; digit_before = false;
                }
                at += num;
                CHECK(got == want && at == x.ext + seed_len + y.ext);
                // a zero right record gives the one-record line
                SamExtend z;
                std::memset(&z, 0, sizeof z);
                CHECK(sam_line_len(L, &x, &z) == sam_line_len(L, &x));
                std::vector<char> one(sam_line_len(L, &x)), two(sam_line_len(L, &x));
                sam_put_line(one.data(), L, name.data(), rname.data(), seq.data(), qual.data(), &x);
                sam_put_line(two.data(), L, name.data(), rname.data(), seq.data(), qual.data(), &x, &z);
                CHECK(one == two);
            }
    }
    CHECK(both_moved > 300 && clip_gone > 30);
}

int main() {
    Seen seen;
    // the BWT of any text will do for FL's arithmetic: the structure reads runs, not a text.  '\x01' the terminator, '$' a separator, N a byte of neither kind
    check_text(std::string("ACGT") + "\x01" + "$$N" + "AAAAAAAACCCCGTGTGTGTACACACAC" + std::string(40, 'T') + "G", seen);     // every base in several runs
    check_text(std::string(37, 'C') + "\x01" + "A" + "$" + "GAGAGAGAGAGAGAGA" + std::string(9, 'A'), seen);                   // C: a single run; T absent
    check_text(std::string("ACACACACACACAC") + "\x01" + "TGTGTGTG$", seen);                                                   // one-symbol runs only: shift 0
    {   // G: 64 symbols in 16 runs (shift 2) with four one-symbol runs in a row (a full bucket), and one run over several buckets
        std::string s = "\x01";
        for (int k = 0; k < 4; ++k) s += "GA";
        s += std::string(49, 'G') + "T";
        for (int k = 0; k < 11; ++k) s += "GC";
        s += "$" + std::string(30, 'A');
        check_text(s, seen);
    }
    {   // many runs behind one long run: buckets of three and more runs are searched
        std::string s = std::string(200, 'A');
        for (int k = 0; k < 25; ++k) s += "CA";
        s += "\x01";
        check_text(s, seen);
    }
    CHECK(seen.single_run && seen.absent && seen.shift0 && seen.full_bucket && seen.run_over_buckets && seen.first_last >= 8 && seen.terminator && seen.separator &&
          seen.search);
    check_huge();
    check_lines();
    std::printf("fl host ok %llu checks\n", g_checks);
    return 0;
}
