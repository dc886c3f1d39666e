// seeds_shim_check -- the reference's GreedyLocateTester (rb_tests.cpp:68-95) through rowbowt_gpu.hpp, as the reference wrote it:
// get_seeds_greedy_w_sample first, locate_from_longest_seed second.  Per query four lines:
//   "seeds <lo,hi,qstart,qend,ssamp> ..."   get_seeds_greedy_w_sample(query, min_length)
//   "plain <lo,hi,qstart,qend> ..."         get_seeds_greedy(query, min_length, lfdata)
//   "locs <loc> ..."                        locate_from_longest_seed(-1, lfs)
//   "batch <lo,hi,qstart,qend,ssamp> ..."   the same list from get_seeds_greedy_batch
// then "chk <records>" = find_range_w_toehold_chkpnts(<chk_read>, <wsize>), and "empty <a> <b>": the sizes of the checkpoint list of
// a read that does not occur and of locate_from_longest_seed on an empty list.
//   seeds_shim_check <index_prefix> <queries, one per line> <min_length> <chk_read> <wsize>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "rowbowt_gpu.hpp"

using RB = rbwt::RowBowt<>;

static void print_list(const char *tag, const std::vector<RB::LFData> &lfs, bool with_ssamp) {
    std::printf("%s", tag);
    for (const auto &lf : lfs) {
        std::printf(" %llu,%llu,%llu,%llu", static_cast<unsigned long long>(lf.rn.first), static_cast<unsigned long long>(lf.rn.second),
                    static_cast<unsigned long long>(lf.qstart), static_cast<unsigned long long>(lf.qend));
        if (with_ssamp) std::printf(",%llu", static_cast<unsigned long long>(lf.ssamp));
    }
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: seeds_shim_check <prefix> <queries> <min_length> <chk_read> <wsize>\n");
        return 2;
    }
    auto rb = rbwt::load_rowbowt<>(argv[1], rbwt::LoadRbwtFlag::SA);
    const uint64_t min_length = std::strtoull(argv[3], nullptr, 10), wsize = std::strtoull(argv[5], nullptr, 10);
    std::ifstream in(argv[2]);
    std::vector<std::string> queries;
    for (std::string q; std::getline(in, q);) queries.push_back(q);
    std::vector<std::vector<RB::LFData>> batch;
    rb.get_seeds_greedy_batch(queries, min_length, true, batch);
    for (size_t i = 0; i < queries.size(); ++i) {
        std::vector<RB::LFData> lfs = rb.get_seeds_greedy_w_sample(queries[i], min_length);   // rb_tests.cpp:76
        print_list("seeds", lfs, true);
        std::vector<RB::LFData> plain;
        print_list("plain", rb.get_seeds_greedy(queries[i], min_length, plain), false);
        std::vector<uint64_t> locs = rb.locate_from_longest_seed(-1, lfs);                     // rb_tests.cpp:77
        std::printf("locs");
        for (const uint64_t l : locs) std::printf(" %llu", static_cast<unsigned long long>(l));
        std::printf("\n");
        print_list("batch", batch[i], true);
    }
    print_list("chk", rb.find_range_w_toehold_chkpnts(argv[4], wsize), true);
    std::printf("empty %zu %zu\n", rb.find_range_w_toehold_chkpnts(std::string(argv[4]) + "N", wsize).size(),
                rb.locate_from_longest_seed(-1, std::vector<RB::LFData>()).size());
    return 0;
}
