// tally_shim_check -- rowbowt_gpu.hpp's MarkerTally once round: the reads of a file (one per line) go through RowBowt::markers_tally in two
// halves with rb_markers' default parameters; the entries, the info and a merge into a second tally are printed for the test to compare with
// the model.
//   tally_shim_check <index_prefix> <queries, one per line>
#include <fstream>

#include "rowbowt_gpu.hpp"

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: tally_shim_check <prefix> <queries>\n");
        return 2;
    }
    rbwt::RowBowt<> rb = rbwt::load_rowbowt<>(argv[1], rbwt::LoadRbwtFlag::MA);
    std::vector<std::string> reads;
    std::ifstream in(argv[2]);
    for (std::string line; std::getline(in, line);) reads.push_back(line);
    rbg_report_params_t p{};
    p.wsize = 19;
    p.max_range = 1000;
    p.read_len = 101;
    {
        rbwt::MarkerTally tally = rb.make_tally(), merged = rb.make_tally(16);
        const size_t half = reads.size() / 2;
        rb.markers_tally(std::vector<std::string>(reads.begin(), reads.begin() + half), p, {}, tally);
        rb.markers_tally(std::vector<std::string>(reads.begin() + half, reads.end()), p, {}, tally);
        const std::vector<rbg_tally_entry_t> e = tally.entries();
        for (const rbg_tally_entry_t &x : e)
            std::printf("entry %llu %llu %llu %llu\n", (unsigned long long)x.marker, (unsigned long long)x.n_fwd, (unsigned long long)x.n_rev,
                        (unsigned long long)x.len_sum);
        const rbwt::MarkerTally::Info i = tally.info();
        std::printf("info %llu %d %llu\n", (unsigned long long)i.entries, i.capacity >= 2 * i.entries, (unsigned long long)i.dropped);
        merged.add_entries(e);
        merged.add_entries(e);
        const std::vector<rbg_tally_entry_t> m = merged.entries();
        bool twice = m.size() == e.size();
        for (size_t j = 0; twice && j < e.size(); ++j)
            twice = m[j].marker == e[j].marker && m[j].n_fwd == 2 * e[j].n_fwd && m[j].n_rev == 2 * e[j].n_rev && m[j].len_sum == 2 * e[j].len_sum;
        std::printf("merged twice %d\n", twice ? 1 : 0);
        tally.reset();
        std::printf("reset %zu\n", tally.entries().size());
    }   // (the tallies go before the index)
    return 0;
}
