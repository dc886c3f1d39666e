// loc_markers_shim_check -- rowbowt_gpu.hpp's rb_locs surface: load_text_markers(<prefix>.midx), then
// find_loc_markers_greedy_seeding_batch over the queries.  Per query two lines:
//   "locs <loc> ..."   its locations (find_locs_greedy_seeding(query, min_length, max_hits))
//   "mk <marker> ..."  the markers over [l, l + len - 1] of every location l, in order
// then "same <0|1>": the batch call returned exactly what rbg_find_loc_markers_greedy_seeding (the C-ABI) returns for the same batch.
//   loc_markers_shim_check <index_prefix> <queries, one per line> <min_length> <max_hits>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "rowbowt_gpu.hpp"

int main(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: loc_markers_shim_check <prefix> <queries> <min_length> <max_hits>\n");
        return 2;
    }
    auto rb = rbwt::load_rowbowt<>(argv[1], rbwt::LoadRbwtFlag::SA | rbwt::LoadRbwtFlag::DL);
    rb.load_text_markers(std::string(argv[1]) + ".midx");
    const uint64_t min_length = std::strtoull(argv[3], nullptr, 10), max_hits = std::strtoull(argv[4], nullptr, 10);
    std::ifstream in(argv[2]);
    std::vector<std::string> queries;
    for (std::string q; std::getline(in, q);) queries.push_back(q);
    std::vector<uint64_t> loc_off, locs, mk_off;
    std::vector<MarkerT> mk;
    rb.find_loc_markers_greedy_seeding_batch(queries, min_length, max_hits, loc_off, locs, mk_off, mk);
    for (size_t i = 0; i < queries.size(); ++i) {
        std::printf("locs");
        for (uint64_t t = loc_off[i]; t < loc_off[i + 1]; ++t) std::printf(" %llu", static_cast<unsigned long long>(locs[t]));
        std::printf("\nmk");
        for (uint64_t t = mk_off[i]; t < mk_off[i + 1]; ++t) std::printf(" %llu", static_cast<unsigned long long>(mk[t]));
        std::printf("\n");
    }
    // the C-ABI call on the same batch
    std::string seqs;
    std::vector<uint64_t> off{0};
    for (const auto &q : queries) { seqs += q; off.push_back(seqs.size()); }
    const uint64_t N = queries.size();
    std::vector<uint64_t> a_loc_off(N + 1), a_mk_off(N + 1);
    uint64_t *a_locs = nullptr, *a_mk = nullptr;
    const int rc = rbg_find_loc_markers_greedy_seeding(rb.handle(), reinterpret_cast<const uint8_t *>(seqs.data()), off.data(), N, min_length, max_hits,
                                                       a_loc_off.data(), &a_locs, a_mk_off.data(), &a_mk);
    bool same = rc == RBG_OK && a_loc_off == loc_off && a_mk_off == mk_off;
    if (same) same = std::vector<uint64_t>(a_locs, a_locs + a_loc_off[N]) == locs && std::vector<uint64_t>(a_mk, a_mk + a_mk_off[N]) == mk;
    rbg_free_buffer(a_locs);
    rbg_free_buffer(a_mk);
    std::printf("same %d\n", same ? 1 : 0);
    return same ? 0 : 1;
}
