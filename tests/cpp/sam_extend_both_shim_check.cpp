// sam_extend_both_shim_check -- rowbowt_gpu.hpp's fl_prepare and align_sam_extend_both, instantiated and run: a document table attached through the C-ABI (names
// d0, d1, ... and the starts as given), the FL index prepared, then the SAM lines of the reads on stdout.
//   sam_extend_both_shim_check <index_prefix> <reads: "name<TAB>seq<TAB>qual" per line> <starts, comma-separated> <min_length> <max_hits> <secondary 0|1> <quals 0|1> <max_mismatch|default>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "rowbowt_gpu.hpp"

int main(int argc, char **argv) {
    if (argc < 9) {
        std::fprintf(stderr, "usage: sam_extend_both_shim_check <prefix> <reads> <starts> <min_length> <max_hits> <secondary> <quals> <max_mismatch|default>\n");
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
    const std::vector<std::string> none;
    rb.fl_prepare();
    rb.fl_prepare();   // (idempotent)
    const std::string text = std::strcmp(argv[8], "default") == 0
                                 ? rb.align_sam_extend_both(seqs, with_quals ? quals : none, names, min_length, max_hits, secondary)
                                 : rb.align_sam_extend_both(seqs, with_quals ? quals : none, names, min_length, max_hits, secondary,
                                                            static_cast<uint32_t>(std::strtoul(argv[8], nullptr, 10)));
    std::fwrite(text.data(), 1, text.size(), stdout);
    return 0;
}
