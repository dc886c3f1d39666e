// rb_extract -- the indexed text as FASTA, read back from the index on the device (rbg_extract; `samtools faidx` on an index whose FASTA is no longer at hand):
//   rb_extract [--all] [--line-width n] [--gpu n] <index_prefix> [region ...]
// A region is `name` (the whole document) or `name:beg-end`, 1-based inclusive, resolved through the document table (rbg_doc_table: document j spans from its
// start to the next sorted start, the last one to the end of the text).  Output: `>name` or `>name:beg-end`, then lines of --line-width bases (default 60).
// The text ends at the first byte that is no base of A C G T: a document is written up to its separator or the terminator; a region that meets such a byte
// before its end, or that reaches past its document, is written up to there, with a warning on stderr.  The index is loaded with SA | DL: a missing .tsa or
// .docs exits 1 ("bad file"), an unknown name exits 1 with a message.
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/rowbowt_gpu.hpp"

namespace {

struct Args {
    std::string inpre;
    std::vector<std::string> regions;
    int all = 0, device = 0;
    uint64_t width = 60;
};

void print_help() {
    fprintf(stderr, "rb_extract\n");
    fprintf(stderr, "Usage: rb_extract [options] <index_prefix> [region ...]\n");
    fprintf(stderr, "    --all                  every document of the index, in the order of their starts\n");
    fprintf(stderr, "    --line-width <int>     bases per line (default 60)\n");
    fprintf(stderr, "    --gpu <n>              HIP device ordinal (default 0)\n");
    fprintf(stderr, "    <region>               name, or name:beg-end (1-based, inclusive)\n");
}

Args parse_args(int argc, char **argv) {
    static Args args;
    static struct option long_options[] = {{"all", no_argument, &args.all, 1},
                                           {"line-width", required_argument, 0, 'w'},
                                           {"gpu", required_argument, 0, 'G'},
                                           {"help", no_argument, 0, 'h'},
                                           {0, 0, 0, 0}};
    int c, long_index = 0;
    while ((c = getopt_long(argc, argv, "hw:", long_options, &long_index)) != -1) {
        switch (c) {
            case 0: break;
            case 'w': {
                char *end = nullptr;
                args.width = std::strtoull(optarg, &end, 10);
                if (end == optarg || *end || args.width == 0) { fprintf(stderr, "rb_extract: --line-width takes a positive number\n"); std::exit(1); }
                break;
            }
            case 'G': args.device = std::atoi(optarg); break;
            case 'h': print_help(); std::exit(0);
            default: print_help(); std::exit(1);
        }
    }
    if (argc - optind < 1) { fprintf(stderr, "no argument provided\n"); print_help(); std::exit(1); }
    args.inpre = argv[optind++];
    for (; optind < argc; ++optind) args.regions.push_back(argv[optind]);
    if (!args.all && args.regions.empty()) { fprintf(stderr, "rb_extract: give a region or --all\n"); std::exit(1); }
    return args;
}

struct Docs {
    uint64_t n = 0, text_n = 0;
    const uint64_t *starts = nullptr;
    const char *const *names = nullptr;
    int64_t find(const std::string &name) const {
        for (uint64_t d = 0; d < n; ++d)
            if (name == names[d]) return static_cast<int64_t>(d);
        return -1;
    }
    uint64_t end(uint64_t d) const { return d + 1 < n ? starts[d + 1] : text_n; }
};

struct Region {
    std::string label;
    uint64_t doc = 0, pos = 0, len = 0;
    bool whole = true;
};

// `name`, else `name:beg-end` split at the last colon (a name may hold colons itself)
bool parse_region(const Docs &docs, const std::string &s, Region &r) {
    r.label = s;
    int64_t d = docs.find(s);
    if (d >= 0) {
        r.doc = static_cast<uint64_t>(d);
        r.pos = docs.starts[d];
        r.len = docs.end(r.doc) - r.pos;
        r.whole = true;
        return true;
    }
    const size_t colon = s.rfind(':');
    if (colon == std::string::npos || (d = docs.find(s.substr(0, colon))) < 0) {
        fprintf(stderr, "rb_extract: no document named '%s' in the index\n", s.substr(0, colon).c_str());
        return false;
    }
    const std::string span = s.substr(colon + 1);
    char *e1 = nullptr, *e2 = nullptr;
    const unsigned long long beg = std::strtoull(span.c_str(), &e1, 10);
    const unsigned long long end = (e1 != span.c_str() && *e1 == '-') ? std::strtoull(e1 + 1, &e2, 10) : 0;
    if (e1 == span.c_str() || *e1 != '-' || e2 == e1 + 1 || *e2 || beg == 0 || end < beg) {
        fprintf(stderr, "rb_extract: '%s' is no region (name:beg-end, 1-based, beg <= end)\n", s.c_str());
        return false;
    }
    r.doc = static_cast<uint64_t>(d);
    const uint64_t extent = docs.end(r.doc) - docs.starts[d];
    if (beg > extent) {
        fprintf(stderr, "rb_extract: '%s' starts beyond its document (%llu positions)\n", s.c_str(), static_cast<unsigned long long>(extent));
        return false;
    }
    r.pos = docs.starts[d] + (beg - 1);
    r.len = end - beg + 1;
    r.whole = false;
    if (r.len > extent - (beg - 1)) {
        fprintf(stderr, "rb_extract: warning: '%s' reaches past its document: written up to its end\n", s.c_str());
        r.len = extent - (beg - 1);
    }
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    const Args args = parse_args(argc, argv);
    rbwt::RowBowt<> rb = rbwt::load_rowbowt<>(args.inpre, rbwt::LoadRbwtFlag::DL | rbwt::LoadRbwtFlag::SA, args.device);
    rbg_info_t info;
    rbwt::detail::check(rbg_info(rb.handle(), &info), "rbg_info");
    Docs docs;
    uint64_t size = 0;
    rbwt::detail::check(rbg_doc_table(rb.handle(), &docs.n, &docs.starts, &docs.names, &size), "rbg_doc_table");
    docs.text_n = info.n;
    std::vector<Region> regions;
    if (args.all)
        for (uint64_t d = 0; d < docs.n; ++d) {
            Region r;
            if (!parse_region(docs, docs.names[d], r)) return 1;
            r.doc = d;                       // (two documents of one name: each its own)
            r.pos = docs.starts[d];
            r.len = docs.end(d) - r.pos;
            regions.push_back(r);
        }
    for (const std::string &s : args.regions) {
        Region r;
        if (!parse_region(docs, s, r)) return 1;
        regions.push_back(r);
    }
    rb.extract_prepare();
    std::vector<uint64_t> pos, len;
    for (const Region &r : regions) { pos.push_back(r.pos); len.push_back(r.len); }
    const auto ex = rb.extract(pos, len);
    for (size_t j = 0; j < regions.size(); ++j) {
        const Region &r = regions[j];
        const std::string &t = ex.text[j];
        // a whole document ends at its separator or at the terminator: only an earlier stop is worth a word
        if (t.size() < r.len && !(r.whole && t.size() + 1 == r.len))
            fprintf(stderr, "rb_extract: warning: '%s' meets a byte that is no base after %llu bases: written up to it\n", r.label.c_str(),
                    static_cast<unsigned long long>(t.size()));
        fputc('>', stdout);
        fputs(r.label.c_str(), stdout);
        fputc('\n', stdout);
        for (size_t at = 0; at < t.size(); at += args.width) {
            fwrite(t.data() + at, 1, std::min<size_t>(args.width, t.size() - at), stdout);
            fputc('\n', stdout);
        }
    }
    return 0;
}
