// doc_hits_shim_check -- rowbowt_gpu.hpp's document surface: a table attached through the C-ABI (names d0, d1, ... and the starts AS GIVEN on the command
// line, so a test can give them out of order), then doc_hits over the queries and the batched resolve_offsets over the positions.  Output:
//   "read <lo> <hi> <ndocs> <nodoc> <set word 0> ..."   per query (doc_hits; the words of its set)
//   "bits <d> ..."                                        per query: the documents DocHits::hit answers true for
//   "reads <doc_reads[0]> ..."                            reads per document
//   "pos <position> <doc | none> <offset> <name | ->"     per position (resolve_offsets)
//   "single <0|1>"                                        every position that has a document agrees with the one-position resolve_offset
//   doc_hits_shim_check <index_prefix> <queries, one per line> <max_hits> <starts, comma-separated> <positions, comma-separated>
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
    if (argc < 6) {
        std::fprintf(stderr, "usage: doc_hits_shim_check <prefix> <queries> <max_hits> <starts> <positions>\n");
        return 2;
    }
    auto rb = rbwt::load_rowbowt<>(argv[1], rbwt::LoadRbwtFlag::SA);
    const uint64_t max_hits = std::strtoull(argv[3], nullptr, 10);
    const std::vector<uint64_t> starts = numbers(argv[4]), positions = numbers(argv[5]);
    std::string names;
    for (size_t j = 0; j < starts.size(); ++j) { names += "d" + std::to_string(j); names.push_back('\0'); }
    if (rbg_set_docs(rb.handle(), names.c_str(), starts.data(), starts.size()) != RBG_OK) return 3;
    std::ifstream in(argv[2]);
    std::vector<std::string> queries;
    for (std::string q; std::getline(in, q);) queries.push_back(q);
    const auto h = rb.doc_hits(queries, max_hits);
    for (size_t i = 0; i < queries.size(); ++i) {
        std::printf("read %llu %llu %u %u", (unsigned long long)h.ranges[i].first, (unsigned long long)h.ranges[i].second, h.ndocs[i], h.nodoc[i]);
        for (uint64_t w = 0; w < h.words; ++w) std::printf(" %llu", (unsigned long long)h.sets[i * h.words + w]);
        std::printf("\nbits");
        for (uint64_t d = 0; d < starts.size(); ++d)
            if (h.hit(i, d)) std::printf(" %llu", (unsigned long long)d);
        std::printf("\n");
    }
    std::printf("reads");
    for (uint64_t c : h.doc_reads) std::printf(" %llu", (unsigned long long)c);
    std::printf("\n");
    const auto r = rb.resolve_offsets(positions);
    bool single = true;
    for (size_t i = 0; i < positions.size(); ++i) {
        if (r.doc[i] == RBG_DOC_NONE) {
            std::printf("pos %llu none %llu -\n", (unsigned long long)positions[i], (unsigned long long)r.offset[i]);
            continue;
        }
        std::printf("pos %llu %u %llu %s\n", (unsigned long long)positions[i], r.doc[i], (unsigned long long)r.offset[i], r.names[r.doc[i]].c_str());
        const auto one = rb.resolve_offset(positions[i]);
        single = single && one.first == r.names[r.doc[i]] && one.second == r.offset[i];
    }
    std::printf("single %d\n", single ? 1 : 0);
    return single ? 0 : 1;
}
