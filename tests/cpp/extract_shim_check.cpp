// The C++ shim's extract_prepare / isa / extract (rowbowt_amd/include/rowbowt_gpu.hpp) on an index with a document list:
//   extract_shim_check <index_prefix> <file with the document's bases>
// extract against the bases given (made by the caller from the BWT, not by the library), single and batched, across the document's end; isa against
// find_range: the row of the suffix at p is the only row of the range of a window long enough to be unique.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "rowbowt_gpu.hpp"

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[2], std::ios::binary);
    const std::string bases((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    CHECK(bases.size() > 1000);
    rbwt::RowBowt<> rb = rbwt::load_rowbowt<>(argv[1], rbwt::LoadRbwtFlag::SA | rbwt::LoadRbwtFlag::DL);
    rb.extract_prepare();
    rb.extract_prepare();      // idempotent
    const uint64_t L = bases.size();
    CHECK(rb.extract(0, 1) == bases.substr(0, 1) && rb.extract(0, L) == bases && rb.extract(L - 1, 1) == bases.substr(L - 1));
    CHECK(rb.extract(L - 10, 500) == bases.substr(L - 10) && rb.extract(L, 5).empty() && rb.extract(17, 0).empty());
    std::vector<uint64_t> pos, len;
    for (uint64_t p = 0; p + 300 < L; p += 997) { pos.push_back(p); len.push_back(1 + p % 300); }
    pos.push_back(L - 3); len.push_back(40);
    const auto ex = rb.extract(pos, len);
    CHECK(ex.text.size() == pos.size() && ex.got.size() == pos.size());
    for (size_t j = 0; j < pos.size(); ++j) {
        const std::string want = bases.substr(pos[j], len[j]);
        CHECK(ex.text[j] == want && ex.got[j] == want.size());
    }
    CHECK(ex.got.back() == 3);
    // isa: a window of 40 bases that occurs once has a one-row range, and that row is the row of its position
    unsigned unique = 0;
    std::vector<uint64_t> ps;
    for (uint64_t p = 0; p + 40 < L; p += 1013) ps.push_back(p);
    const std::vector<uint64_t> rows = rb.isa(ps);
    for (size_t j = 0; j < ps.size(); ++j) {
        const auto rn = rb.find_range(bases.substr(ps[j], 40));
        CHECK(rn.first <= rows[j] && rows[j] <= rn.second);
        unique += rn.first == rn.second;
    }
    CHECK(unique > 0 && rb.isa(ps[1]) == rows[1]);
    std::printf("extract shim ok: %zu intervals, %zu positions (%u with a one-row range)\n", pos.size(), ps.size(), unique);
    return 0;
}
