// locate_doc_hits_shim_check -- rowbowt_gpu.hpp's doc_hits overloads that return the locations per document (rbg_doc_hits_locs): a table attached through
// the C-ABI (names d0, d1, ... and the starts AS GIVEN on the command line), then doc_hits over the queries with doc_locs, and without it for comparison.
// Output:
//   "read <lo> <hi> <ndocs> <nodoc> <set word 0> ..."   per query
//   "reads <doc_reads[0]> ..."                            reads per document
//   "locs <doc_locs[0]> ..."                              locations per document
//   "same <0|1>"                                          the overload without doc_locs gives the same other outputs; the unlimited overload equals max_hits = 2^64 - 1
//   locate_doc_hits_shim_check <index_prefix> <queries, one per line> <max_hits> <starts, comma-separated>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "rowbowt_gpu.hpp"

static std::vector<uint64_t> numbers(const char *arg) {
    std::vector<uint64_t> v;
    std::stringstream ss(arg);
    for (std::string t; std::getline(ss, t, ',');) v.push_back(std::strtoull(t.c_str(), nullptr, 10));
    return v;
}

int main(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: locate_doc_hits_shim_check <prefix> <queries> <max_hits> <starts>\n");
        return 2;
    }
    auto rb = rbwt::load_rowbowt<>(argv[1], rbwt::LoadRbwtFlag::SA);
    const uint64_t max_hits = std::strtoull(argv[3], nullptr, 10);
    const std::vector<uint64_t> starts = numbers(argv[4]);
    std::string names;
    for (size_t j = 0; j < starts.size(); ++j) { names += "d" + std::to_string(j); names.push_back('\0'); }
    if (rbg_set_docs(rb.handle(), names.c_str(), starts.data(), starts.size()) != RBG_OK) return 3;
    std::ifstream in(argv[2]);
    std::vector<std::string> queries;
    for (std::string q; std::getline(in, q);) queries.push_back(q);
    std::vector<uint64_t> doc_locs(3, 99);   // (assigned, whatever it held)
    const auto h = rb.doc_hits(queries, max_hits, doc_locs);
    for (size_t i = 0; i < queries.size(); ++i) {
        std::printf("read %llu %llu %u %u", (unsigned long long)h.ranges[i].first, (unsigned long long)h.ranges[i].second, h.ndocs[i], h.nodoc[i]);
        for (uint64_t w = 0; w < h.words; ++w) std::printf(" %llu", (unsigned long long)h.sets[i * h.words + w]);
        std::printf("\n");
    }
    std::printf("reads");
    for (uint64_t c : h.doc_reads) std::printf(" %llu", (unsigned long long)c);
    std::printf("\nlocs");
    for (uint64_t c : doc_locs) std::printf(" %llu", (unsigned long long)c);
    std::printf("\n");
    const auto plain = rb.doc_hits(queries, max_hits);
    bool same = plain.sets == h.sets && plain.ndocs == h.ndocs && plain.nodoc == h.nodoc && plain.doc_reads == h.doc_reads && plain.ranges == h.ranges;
    if (max_hits == static_cast<uint64_t>(-1)) {
        std::vector<uint64_t> again;
        const auto all = rb.doc_hits(queries, again);
        same = same && again == doc_locs && all.sets == h.sets;
    }
    std::printf("same %d\n", same ? 1 : 0);
    return same ? 0 : 1;
}
