// tally_reads_shim_check -- rowbowt_gpu.hpp's MarkerTally in per-read mode: the reads of a file (one per line) go through RowBowt::markers_tally
// with a flag word (RBG_TALLY_PER_READ [| RBG_TALLY_DROP_SITE_CONFLICTS]) in two halves; the entries, the info's elements and the read_info are
// printed for the test to compare with the model.
//   tally_reads_shim_check <index_prefix> <queries, one per line> <wsize> <tally_flags>
#include <cstdlib>
#include <fstream>

#include "rowbowt_gpu.hpp"

int main(int argc, char **argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: tally_reads_shim_check <prefix> <queries> <wsize> <tally_flags>\n");
        return 2;
    }
    rbwt::RowBowt<> rb = rbwt::load_rowbowt<>(argv[1], rbwt::LoadRbwtFlag::MA);
    std::vector<std::string> reads;
    std::ifstream in(argv[2]);
    for (std::string line; std::getline(in, line);) reads.push_back(line);
    rbg_report_params_t p{};
    p.wsize = std::strtoull(argv[3], nullptr, 10);
    p.max_range = 1000;
    p.read_len = 101;
    const uint32_t flags = static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 10));
    {
        rbwt::MarkerTally tally = rb.make_tally();
        const size_t half = reads.size() / 2;
        rb.markers_tally(std::vector<std::string>(reads.begin(), reads.begin() + half), p, {}, tally, flags);
        rb.markers_tally(std::vector<std::string>(reads.begin() + half, reads.end()), p, {}, tally, flags);
        for (const rbg_tally_entry_t &x : tally.entries())
            std::printf("entry %llu %llu %llu %llu\n", (unsigned long long)x.marker, (unsigned long long)x.n_fwd, (unsigned long long)x.n_rev,
                        (unsigned long long)x.len_sum);
        const rbwt::MarkerTally::Info i = tally.info();
        const rbwt::MarkerTally::ReadInfo r = tally.read_info();
        std::printf("elements %llu\n", (unsigned long long)i.elements);
        std::printf("read_info %llu %llu %llu %llu\n", (unsigned long long)r.reads, (unsigned long long)r.elements_seen, (unsigned long long)r.lost,
                    (unsigned long long)r.site_dropped);
        tally.reset();
        const rbwt::MarkerTally::ReadInfo z = tally.read_info();
        std::printf("reset %zu %llu\n", tally.entries().size(), (unsigned long long)(z.reads + z.elements_seen + z.lost + z.site_dropped));
    }   // (the tally goes before the index)
    return 0;
}
