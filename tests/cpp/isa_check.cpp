// The ISA sample that host and device share (rowbowt_amd/csrc/rbg_isa.hpp), on the host: isa_build from the run arrays and toehold samples of small texts
// (made here from a naive suffix array, as the host index holds them), isa_lookup and isa_row at every position against the naive ISA at both position widths,
// on inputs that hold every shape the structure distinguishes (each asserted present); and 8-byte positions over a synthetic sample list with samples on
// both sides of 2^32, lookup only.  Stand-alone: g++ -fsanitize=address,undefined tests/cpp/isa_check.cpp.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../rowbowt_amd/csrc/rbg_isa.hpp"

using namespace rbg;

static unsigned long long g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

// what the shapes below must show at least once
struct Seen {
    unsigned shift0 = 0, empty_bucket = 0, bisected = 0, first_last = 0, interior_other = 0, second_kind = 0;
    unsigned long_other_run = 0;      // a non-base BWT run of at least 16 rows
    unsigned other_pair = 0;          // two non-base bytes side by side in the text
};

struct Host {      // what HostIndex holds of a text
    uint64_t n = 0;
    std::vector<uint64_t> sa, isa;
    std::string bwt;
    std::vector<uint8_t> heads;
    std::vector<uint64_t> run_start, samples_last, pred_pos, phi_base;
    uint64_t F[256];
};

static Host host_of(const std::string &text) {
    Host h;
    const uint64_t n = h.n = text.size();
    CHECK(n >= 2 && text[n - 1] == '\x01' && text.find('\x01') == n - 1);
    h.sa.resize(n);
    std::iota(h.sa.begin(), h.sa.end(), uint64_t(0));
    std::sort(h.sa.begin(), h.sa.end(), [&](uint64_t a, uint64_t b) { return text.compare(a, std::string::npos, text, b, std::string::npos) < 0; });
    h.isa.resize(n);
    for (uint64_t i = 0; i < n; ++i) h.isa[h.sa[i]] = i;
    for (uint64_t i = 0; i < n; ++i) h.bwt.push_back(text[(h.sa[i] + n - 1) % n]);
    std::vector<uint64_t> first_sample;      // SA - 1 at the first row of every run
    for (uint64_t i = 0; i < n; ++i) {
        if (i == 0 || h.bwt[i] != h.bwt[i - 1]) {
            h.heads.push_back(static_cast<uint8_t>(h.bwt[i]));
            h.run_start.push_back(i);
            first_sample.push_back((h.sa[i] + n - 1) % n);
        }
        if (i + 1 == n || h.bwt[i + 1] != h.bwt[i]) h.samples_last.push_back((h.sa[i] + n - 1) % n);
    }
    h.run_start.push_back(n);
    const uint64_t R = h.heads.size();
    std::vector<uint64_t> order(R);
    std::iota(order.begin(), order.end(), uint64_t(0));
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return first_sample[a] < first_sample[b]; });
    for (uint64_t j = 0; j < R; ++j) {
        h.pred_pos.push_back(first_sample[order[j]]);
        h.phi_base.push_back(order[j] ? h.samples_last[order[j] - 1] : 0);      // toehold_sa.hpp:67-70
    }
    uint64_t count[256] = {}, acc = 0;
    for (char c : text) count[static_cast<uint8_t>(c)] += 1;
    for (int c = 0; c < 256; ++c) { h.F[c] = acc; acc += count[c]; }
    return h;
}

template <typename P>
static void check_index(const Host &h, const IsaIndex &X, const FlIndex &FLX, Seen &seen) {
    const uint64_t n = h.n, S = X.samples;
    const IsaEnt<P> *ent = reinterpret_cast<const IsaEnt<P> *>(X.blob.data());
    const P *dir = reinterpret_cast<const P *>(X.blob.data() + X.dir_at);
    CHECK(X.n == n && X.pos_bytes == sizeof(P) && X.bytes() == isa_bytes(n, S, sizeof(P)) && X.bytes() == S * 2 * sizeof(P) + X.dir_entries * sizeof(P));
    CHECK((S << X.shift) <= n && (S << (X.shift + 1)) > n && X.dir_entries == (n >> X.shift) + 2);
    seen.shift0 += X.shift == 0;
    // the samples: suffix array pairs, ascending and distinct, position 0 first; the runs' last rows and the other rows of the non-base runs, nothing else
    std::vector<char> is_sample_row(n, 0);
    uint64_t gap = 0;
    for (uint64_t j = 0; j < S; ++j) {
        CHECK(ent[j].row < n && h.sa[ent[j].row] == ent[j].tpos && (j == 0 ? ent[j].tpos == 0 : ent[j].tpos > ent[j - 1].tpos));
        is_sample_row[ent[j].row] = 1;
        gap = std::max<uint64_t>(gap, (j + 1 < S ? static_cast<uint64_t>(ent[j + 1].tpos) : n) - ent[j].tpos);
    }
    CHECK(gap == X.max_gap);
    uint64_t second = 0;
    for (uint64_t g = 0; g + 1 < h.run_start.size(); ++g) {
        seen.long_other_run += !isa_is_base(h.heads[g]) && h.run_start[g + 1] - h.run_start[g] >= 16;
        for (uint64_t row = h.run_start[g]; row < h.run_start[g + 1]; ++row) {
            const bool last = row + 1 == h.run_start[g + 1], other = !isa_is_base(h.heads[g]);
            CHECK(is_sample_row[row] == ((last || other) ? 1 : 0));
            second += other && !last;
            seen.interior_other += other && !last && row > h.run_start[g];      // neither the first nor the last row of its run
        }
    }
    CHECK(second == X.second_kind && S == h.heads.size() + second);
    seen.second_kind += second > 0;
    // the directory: dir[b] = the largest sample at or before b << shift
    for (uint64_t b = 0; b < X.dir_entries; ++b) {
        const uint64_t at = b << X.shift;
        CHECK(dir[b] < S && ent[dir[b]].tpos <= at && (dir[b] + 1 == S || ent[dir[b] + 1].tpos > at));
        if (b + 1 < X.dir_entries && at < n) {
            bool any = false;
            for (uint64_t j = 0; j < S; ++j) any = any || (ent[j].tpos >= at && ent[j].tpos < ((b + 1) << X.shift));
            seen.empty_bucket += !any;
        }
    }
    // every position: the lookup against a scan, the row against the naive ISA
    const IsaView v = X.view(X.blob.data());
    const FlView fl = FLX.view(FLX.blob.data());
    for (uint64_t p = 0; p < n; ++p) {
        uint64_t want = 0;
        for (uint64_t j = 0; j < S && ent[j].tpos <= p; ++j) want = j;
        unsigned long long probes = 0;
        const IsaHit hit = isa_lookup<P>(v, p, &probes);
        CHECK(hit.tpos == ent[want].tpos && hit.row == ent[want].row && p - hit.tpos < X.max_gap);
        seen.bisected += probes > 0;
        CHECK(isa_row<P>(v, fl, p) == h.isa[p]);
        seen.first_last += p == 0 || p == n - 1;
    }
}

static void check_text(const std::string &text, Seen &seen) {
    const Host h = host_of(text);
    for (size_t i = 0; i + 2 < text.size(); ++i)
        seen.other_pair += !isa_is_base(static_cast<uint8_t>(text[i])) && !isa_is_base(static_cast<uint8_t>(text[i + 1]));
    for (uint32_t pb : {4u, 8u}) {
        IsaIndex X;
        FlIndex FLX;
        CHECK(isa_build(h.heads.data(), h.run_start.data(), h.heads.size(), h.samples_last.data(), h.pred_pos.data(), h.phi_base.data(), pb, X));
        CHECK(fl_build(h.heads.data(), h.run_start.data(), h.heads.size(), h.F, pb, FLX));
        if (pb == 4) check_index<uint32_t>(h, X, FLX, seen); else check_index<uint64_t>(h, X, FLX, seen);
    }
}

// 8-byte positions, samples on both sides of 2^32: the lookup alone over a synthetic list
static void check_wide() {
    const uint64_t n = (uint64_t(1) << 33) + 12345, two32 = uint64_t(1) << 32;
    std::vector<IsaPair> s;
    uint64_t x = 88172645463325252ull, row = 0;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    s.push_back(IsaPair{0, row++});
    for (uint64_t d = 0; d < 40; ++d) { s.push_back(IsaPair{two32 - 1 - 3 * d, row++}); s.push_back(IsaPair{two32 + 5 * d, row++}); }
    for (int i = 0; i < 3000; ++i) s.push_back(IsaPair{1 + rnd() % (n - 1), row++});
    std::sort(s.begin(), s.end(), [](const IsaPair &a, const IsaPair &b) { return a.tpos < b.tpos; });
    s.erase(std::unique(s.begin(), s.end(), [](const IsaPair &a, const IsaPair &b) { return a.tpos == b.tpos; }), s.end());
    std::vector<IsaPair> shuffled(s.rbegin(), s.rend());
    IsaIndex X;
    CHECK(!isa_build_pairs(shuffled, n, 4, 0, X));      // 4-byte positions do not hold this n
    shuffled.assign(s.rbegin(), s.rend());
    CHECK(isa_build_pairs(shuffled, n, 8, 0, X));
    CHECK(X.samples == s.size() && X.bytes() == isa_bytes(n, s.size(), 8) && X.shift > 0);
    const IsaView v = X.view(X.blob.data());
    std::vector<uint64_t> ps = {0, 1, n - 1, n - 2, two32 - 1, two32, two32 + 1};
    for (const IsaPair &e : s) { ps.push_back(e.tpos); if (e.tpos) ps.push_back(e.tpos - 1); if (e.tpos + 1 < n) ps.push_back(e.tpos + 1); }
    for (uint64_t b = 0; b + 1 < X.dir_entries; ++b) { if ((b << X.shift) < n) ps.push_back(b << X.shift); if (((b + 1) << X.shift) - 1 < n) ps.push_back(((b + 1) << X.shift) - 1); }
    bool low = false, high = false, across = false;
    for (const uint64_t p : ps) {
        const auto it = std::upper_bound(s.begin(), s.end(), p, [](uint64_t q, const IsaPair &e) { return q < e.tpos; }) - 1;
        const IsaHit hit = isa_lookup<uint64_t>(v, p);
        CHECK(hit.tpos == it->tpos && hit.row == it->row);
        low = low || hit.tpos < two32;
        high = high || hit.tpos >= two32;
        across = across || (p >= two32 && hit.tpos < two32);
    }
    CHECK(low && high);
    (void)across;
    // what the builder refuses: no sample at 0, two samples at one position, a position >= n
    std::vector<IsaPair> bad = {{5, 0}, {9, 1}};
    CHECK(!isa_build_pairs(bad, 100, 8, 0, X));
    bad = {{0, 0}, {9, 1}, {9, 2}};
    CHECK(!isa_build_pairs(bad, 100, 8, 0, X));
    bad = {{0, 0}, {100, 1}};
    CHECK(!isa_build_pairs(bad, 100, 8, 0, X));
}

int main() {
    Seen seen;
    uint64_t x = 2463534242ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    auto random_bases = [&](size_t m) { std::string s; for (size_t i = 0; i < m; ++i) s.push_back("ACGT"[rnd() & 3]); return s; };
    check_text(std::string("A\x01", 2), seen);
    check_text(random_bases(70) + '\x01', seen);                                   // nearly every row ends a run: shift 0
    const std::string unit = random_bases(90);
    std::string rep;
    for (int k = 0; k < 6; ++k) { std::string u = unit; u[(k * 13) % 90] = "ACGT"[k & 3]; rep += u; }
    check_text(rep + '\x01', seen);                                                // few runs: wide buckets, most of them empty
    std::string docs = unit + "#N" + unit.substr(10, 60) + "NNNNN" + unit.substr(40, 45) + "#" + unit.substr(0, 30) + "N" + unit.substr(31) + "#" + unit;
    check_text(docs + '\x01', seen);                                               // separators, a run of N, a document that starts with N
    check_text(std::string("NNNNNNNN") + unit + unit + "NNNNNNNN" + unit + '\x01', seen);
    // a collection of near copies: 40 documents of 60 bases with two substitutions each, joined by '#'; every 7th starts with N (the text itself too), every
    // 11th ends with N ("N#"), every 5th holds a run of 1 to 9 N, and one document is empty ("##")
    const std::string stem = random_bases(60);
    std::string many;
    for (int d = 0; d < 40; ++d) {
        std::string u = stem;
        for (int k = 0; k < 2; ++k) { const size_t at = rnd() % 60; u[at] = "ACGT"[(std::string("ACGT").find(u[at]) + 1 + rnd() % 3) & 3]; }
        if (d % 5 == 0) u.replace(10 + rnd() % 30, 1 + (d * 3) % 9, std::string(1 + (d * 3) % 9, 'N'));
        if (d % 7 == 0) u[0] = 'N';
        if (d % 11 == 0) u[u.size() - 1] = 'N';
        if (d) many += '#';
        if (d == 17) many += '#';
        many += u;
    }
    CHECK(many[0] == 'N' && many.find("##") != std::string::npos && many.find("N#") != std::string::npos && many.find("NNNNNNN") != std::string::npos);
    const Seen before_many = seen;
    check_text(many + '\x01', seen);
    CHECK(seen.long_other_run > before_many.long_other_run && seen.other_pair > before_many.other_pair);
    CHECK(seen.long_other_run && seen.other_pair);
    CHECK(seen.shift0 && seen.empty_bucket && seen.bisected && seen.first_last && seen.interior_other && seen.second_kind);
    check_wide();
    std::printf("isa host ok %llu checks\n", g_checks);
    return 0;
}
