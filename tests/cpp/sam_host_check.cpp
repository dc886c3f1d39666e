// sam_host_check.cpp -- rbg_sam.hpp on the host (tests/test_sam_host.py builds this with ASan + UBSan): the complement table, CIGAR text and length,
// sam_line_len against the line sam_put_line formats (and both against a line put together with snprintf), the header text.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../rowbowt_amd/csrc/rbg_sam.hpp"

using namespace rbg;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); if (++fails > 20) std::exit(1); } } while (0)

static std::string dec(unsigned long long v) {
    char b[32];
    std::snprintf(b, sizeof b, "%llu", v);
    return b;
}
static std::string cigar_ref(uint64_t m, uint64_t a, uint64_t b) {
    std::string s;
    if (a) s += dec(a) + "S";
    s += dec(b - a) + "M";
    if (m > b) s += dec(m - b) + "S";
    return s;
}
static std::string revcomp_ref(const std::string &q) {
    std::string r(q.rbegin(), q.rend());
    for (char &c : r) {
        const char *from = "ACGTacgt", *to = "TGCAtgca";
        const char *p = c ? std::strchr(from, c) : nullptr;
        if (p) c = to[p - from];
    }
    return r;
}
// the line by string concatenation, independent of sam_put_line
static std::string line_ref(const SamLine &L, const std::string &name, const std::string &rname, const std::string &seq, const std::string &qual) {
    const bool star = (L.mapped && L.hit > 1) || L.m == 0;
    if (!L.mapped)
        return name + "\t4\t*\t0\t0\t*\t*\t0\t0\t" + (star ? "*" : seq) + "\t" + (star || !L.has_qual ? "*" : qual) + "\n";
    const unsigned flag = (L.reverse ? 16u : 0u) | (L.hit > 1 ? 256u : 0u);
    const std::string s = L.reverse ? revcomp_ref(seq) : seq, q = L.reverse ? std::string(qual.rbegin(), qual.rend()) : qual;
    return name + "\t" + dec(flag) + "\t" + rname + "\t" + dec(L.pos) + "\t255\t" + cigar_ref(L.m, L.a, L.b) + "\t*\t0\t0\t" + (star ? "*" : s) + "\t" +
           (star || !L.has_qual ? "*" : q) + "\tNH:i:" + dec(L.occ) + "\tHI:i:" + dec(L.hit) + "\n";
}

int main() {
    unsigned long long checks = 0;
    // complement: all 256 bytes; an involution on ACGTacgt, the identity elsewhere
    for (int c = 0; c < 256; ++c) {
        const char *from = "ACGTacgt", *to = "TGCAtgca";
        const char *p = c ? std::strchr(from, c) : nullptr;
        const uint8_t want = p ? static_cast<uint8_t>(to[p - from]) : static_cast<uint8_t>(c);
        CHECK(sam_comp(static_cast<uint8_t>(c)) == want);
        CHECK(sam_comp(sam_comp(static_cast<uint8_t>(c))) == c);
        if (!p) CHECK(sam_comp(static_cast<uint8_t>(c)) == c);
        ++checks;
    }
    CHECK(sam_comp('N') == 'N' && sam_comp('n') == 'n');
    // CIGAR: a and m - b in {0, 1, 9, 10}, b - a at the powers of ten (and one less)
    const uint64_t edge[4] = {0, 1, 9, 10};
    for (uint64_t a : edge)
        for (uint64_t t : edge)
            for (int k = 0; k < 20; ++k) {
                uint64_t len = 1;
                for (int j = 0; j < k; ++j) len *= 10;
                for (uint64_t l : {len, len > 1 ? len - 1 : len}) {
                    const uint64_t b = a + l, m = b + t;
                    const std::string want = cigar_ref(m, a, b);
                    std::vector<char> buf(want.size() + 2, '#');
                    const uint32_t n = sam_put_cigar(buf.data() + 1, m, a, b);
                    CHECK(n == want.size() && n == sam_cigar_len(m, a, b));
                    CHECK(std::memcmp(buf.data() + 1, want.data(), want.size()) == 0 && buf.front() == '#' && buf.back() == '#');
                    ++checks;
                }
            }
    // whole lines: sam_line_len == what sam_put_line writes == the reference line; sentinels on both sides intact
    const std::string seqs[] = {"", "A", "ACGTNacgtn", "GATTACAGATTACAGATTACAGATTACA", std::string(300, 'C') + "TTGNA"};
    const std::string names[] = {"", "r", std::string(300, 'x')};
    const uint64_t decs[] = {1, 9, 10, 99, 100, 999999999ull, 1000000000ull, 18446744073709551615ull};
    for (const std::string &seq : seqs)
        for (const std::string &name : names)
            for (const std::string &rname : names)
                for (int kind = 0; kind < 5; ++kind)          // unmapped; forward / reverse primary; forward / reverse secondary
                    for (int hq = 0; hq < 2; ++hq)
                        for (uint64_t v : decs) {
                            std::string qual(seq.size(), '!');
                            for (size_t j = 0; j < qual.size(); ++j) qual[j] = static_cast<char>('!' + j % 90);
                            SamLine L{};
                            L.name_len = name.size();
                            L.mapped = kind > 0;
                            if (L.mapped && seq.empty()) continue;   // (a mapped read has a seed of at least one base)
                            L.reverse = kind == 2 || kind == 4;
                            L.hit = kind >= 3 ? (v > 1 ? v : 2) : 1;
                            L.occ = kind >= 3 ? L.hit : v;
                            L.rname_len = rname.size();
                            L.pos = v;
                            L.m = seq.size();
                            L.a = L.m > 2 ? v % (L.m - 1) : 0;
                            L.b = L.mapped ? L.a + 1 + (v % (L.m - L.a)) : 0;
                            L.has_qual = hq != 0;
                            const std::string want = line_ref(L, name, rname, seq, qual);
                            CHECK(sam_line_len(L) == want.size());
                            std::vector<char> buf(want.size() + 2, '#');
                            sam_put_line(buf.data() + 1, L, name.data(), rname.data(), seq.data(), L.has_qual ? qual.data() : nullptr);
                            CHECK(std::memcmp(buf.data() + 1, want.data(), want.size()) == 0 && buf.front() == '#' && buf.back() == '#');
                            ++checks;
                        }
    // the header: 1, 2 and 1 024 documents, names of length 0 and 300, the last document's length from n, a start beyond n, a PG line
    {
        CHECK(sam_header_text({"only"}, {0}, 100, nullptr) == "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:only\tLN:100\n");
        CHECK(sam_header_text({"", std::string(300, 'n')}, {7, 50}, 80, "@PG\tID:x\n") ==
              "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:\tLN:43\n@SQ\tSN:" + std::string(300, 'n') + "\tLN:30\n@PG\tID:x\n");
        CHECK(sam_header_text({"a", "b"}, {0, 90}, 80, "") == "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:a\tLN:90\n@SQ\tSN:b\tLN:0\n");
        // unsorted input starts: the caller hands over the sorted starts, names in the given order (as the document table pairs them)
        std::vector<uint64_t> given = {500, 0, 200}, sorted = given;
        std::sort(sorted.begin(), sorted.end());
        CHECK(sam_header_text({"x", "y", "z"}, sorted, 600, nullptr) == "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:x\tLN:200\n@SQ\tSN:y\tLN:300\n@SQ\tSN:z\tLN:100\n");
        std::vector<std::string> nm;
        std::vector<uint64_t> st;
        std::string want = "@HD\tVN:1.6\tSO:unsorted\n";
        for (uint64_t j = 0; j < 1024; ++j) {
            nm.push_back("d" + dec(j));
            st.push_back(j * j * 3);
            const uint64_t end = j + 1 < 1024 ? (j + 1) * (j + 1) * 3 : 4000000;
            want += "@SQ\tSN:d" + dec(j) + "\tLN:" + dec(end - j * j * 3) + "\n";
        }
        CHECK(sam_header_text(nm, st, 4000000, nullptr) == want);
        checks += 5;
    }
    if (fails) return 1;
    std::printf("sam host ok %llu\n", checks);
    return 0;
}
