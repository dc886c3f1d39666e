// sam_shim_check -- rowbowt_gpu.hpp's align_sam and sam_header, instantiated and run: a document table attached through the C-ABI (names d0, d1, ... and the
// starts as given), then the header followed by the SAM lines of the reads on stdout.
//   sam_shim_check <index_prefix> <reads: "name<TAB>seq<TAB>qual" per line> <starts, comma-separated> <min_length> <max_hits> <secondary 0|1> <quals 0|1>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "rowbowt_gpu.hpp"

int main(int argc, char **argv) {
    if (argc < 8) {
        std::fprintf(stderr, "usage: sam_shim_check <prefix> <reads> <starts> <min_length> <max_hits> <secondary> <quals>\n");
        return 2;
    }
    auto rb = rbwt::load_rowbowt<>(argv[1], rbwt::LoadRbwtFlag::SA);
    std::vector<uint64_t> starts;
    {
        std::stringstream ss(argv[3]);
        for (std::string t; std::getline(ss, t, ',');) starts.push_back(std::strtoull(t.c_str(), nullptr, 10));
    }
    std::string dnames;
    for (size_t j = 0; j < starts.size(); ++j) { dnames += "d" + std::to_string(j); dnames.push_back('\0'); }
    if (rbg_set_docs(rb.handle(), dnames.c_str(), starts.data(), starts.size()) != RBG_OK) return 3;
    std::vector<std::string> names, seqs, quals;
    std::ifstream in(argv[2]);
    for (std::string line; std::getline(in, line);) {
        const size_t a = line.find('\t'), b = line.find('\t', a + 1);
        names.push_back(line.substr(0, a));
        seqs.push_back(line.substr(a + 1, b - a - 1));
        quals.push_back(line.substr(b + 1));
    }
    const uint64_t min_length = std::strtoull(argv[4], nullptr, 10), max_hits = std::strtoull(argv[5], nullptr, 10);
    const bool secondary = argv[6][0] == '1', with_quals = argv[7][0] == '1';
    const std::string header = rb.sam_header("@PG\tID:sam_shim_check\n");
    const std::string text = with_quals ? rb.align_sam(seqs, quals, names, min_length, max_hits, secondary)
                                        : (secondary || min_length != 20 || max_hits != 16 ? rb.align_sam(seqs, {}, names, min_length, max_hits, secondary)
                                                                                            : rb.align_sam(seqs, names));
    std::fwrite(header.data(), 1, header.size(), stdout);
    std::fwrite(text.data(), 1, text.size(), stdout);
    return 0;
}
