// rb_build -- the reference's index builder CLI (reference src/rb_build.cpp) for this engine:
//   rb_build [-o out_prefix] [-s] [-m] [-l] [-f [-k K]] [-a] <input_prefix>
//   rb_build --fasta <ref.fa[.gz]> -o out_prefix [-s] [-l] [-f [-k K]] [--gpu n]
//   rb_build --fasta <ref.fa[.gz]> --vcf <calls.vcf[.gz]> [--samples a,b,...] [--ma-wsize w] -m -o out_prefix [-s] [-l] [-f [-k K]] [--gpu n]
// reads <input_prefix>.bwt (+ .ssa/.esa with -s, + .docs with -l) exactly as the reference's
// constructors do (rle_string.hpp:44-97, toehold_sa.hpp:27-35,133-155) and writes the engine's
// native cache <out_prefix>.rbgpu, which rb_align / rb_markers / rbg_load pick up when no .rbwt is
// there.  -f / -a write the reference's own text <out_prefix>.ftab (rowbowt.hpp:726-744,
// ftab.hpp:29-34), computed on the GPU.
//
// Differences, all reported on stderr:
//   -m   the reference parses the raw <input_prefix>.ma with pfbwt-f's MarkerArray constructor, which
//        is not vendored; here -m folds an already serialised <input_prefix>.mab into the cache.
//   -x   fbb_string indexes are not supported.
//   --fasta  the reference has no builder from a sequence file (its inputs are pfbwt-f's).  Here the text of the FASTA (rbg_fasta_text.hpp: documents joined
//        by '#', a final 0x01) goes to the device, which makes the suffix array, the runs and the samples (rbg_convert_text); -l writes <out>.docs and
//        stores it in the cache; -m alone is refused: a FASTA carries no markers.
//   --vcf  with --fasta and -m: the documents are the reference's contigs and every selected sample's haplotypes (rbg_vcf.hpp: phased single-base variants
//        applied; indels, symbolic alleles, unknown contigs and duplicate positions are skipped and counted on stderr), and the marker array is built on the
//        device from one site record per document and site with windows of --ma-wsize (default 10) bases (rbg_convert_text_markers).  The cache has no field
//        for the window: it is stored as rbg_convert_runs_markers stores it.  Not built: indels, the text-keyed .midx of rb_locs, a text beyond the device.
//   The sdsl-serialised .rbwt/.tsa are not written (this engine does not need them; an existing
//   reference-built index converts with `rb_build --from-index <prefix>`).
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/rbg.h"
#include "rbg_fasta_text.hpp"
#include "rbg_vcf.hpp"

namespace {

struct Args {  // RowBowtConstructArgs, rowbowt_io.hpp:30-47
    std::string prefix, inpre, fasta, vcf, samples;
    int has_samples = 0, has_wsize = 0;
    uint64_t ma_wsize = 10;
    int ma = 0, tsa = 0, dl = 0, ft = 0, ft_only = 0, fbb = 0, from_index = 0, device = 0;
    uint64_t k = 10;
};

void print_help() {  // rb_build.cpp:11-20
    fprintf(stderr, "rb_build\n");
    fprintf(stderr, "Usage: rb_build [options] <index_prefix>\n");
    fprintf(stderr, "    --output-prefix/-o <basename>    output prefix\n");
    fprintf(stderr, "    --tsa/-s                         build toehold suffix array (<pre>.ssa, <pre>.esa)\n");
    fprintf(stderr, "    --ma/-m                          include the marker array (<pre>.mab)\n");
    fprintf(stderr, "    --dl/-l                          include the document list (<pre>.docs)\n");
    fprintf(stderr, "    --ft/-f [-k <int>]               construct offset table <out>.ftab\n");
    fprintf(stderr, "    --ftab-only/-a                   only construct the offset table from an existing index\n");
    fprintf(stderr, "    --from-index                     convert <pre>.rbwt/.tsa/.mab/.docs instead of raw inputs\n");
    fprintf(stderr, "    --fasta <ref.fa[.gz]>            build from a FASTA on the GPU (needs -o; no <index_prefix>; -m only with --vcf)\n");
    fprintf(stderr, "    --vcf <calls.vcf[.gz]>           with --fasta and -m: index the reference and the samples' haplotypes, and build the marker\n");
    fprintf(stderr, "                                     array on the GPU (phased single-base variants; indels, symbolic alleles, unknown contigs and\n");
    fprintf(stderr, "                                     duplicate positions are skipped and counted; no .midx for rb_locs; the text must fit the device)\n");
    fprintf(stderr, "    --samples <a,b,...>              the samples of the VCF to take (default: all), in VCF column order\n");
    fprintf(stderr, "    --ma-wsize <w>                   marker window, 1..64 bases (default 10)\n");
    fprintf(stderr, "    --gpu <n>                        HIP device ordinal for -f/-a/--fasta (default 0)\n");
    fprintf(stderr, "    <input_prefix>                   index prefix\n");
}

Args parse_args(int argc, char **argv) {  // rb_build.cpp:22-95
    static Args args;
    static struct option long_options[] = {{"output-prefix", required_argument, 0, 'o'},
                                           {"tsa", no_argument, 0, 's'},
                                           {"dl", no_argument, 0, 'l'},
                                           {"ftab-only", no_argument, 0, 'a'},
                                           {"ma", no_argument, 0, 'm'},
                                           {"ft", no_argument, 0, 'f'},
                                           {"fbb", no_argument, 0, 'x'},
                                           {"from-index", no_argument, &args.from_index, 1},
                                           {"gpu", required_argument, 0, 'G'},
                                           {"fasta", required_argument, 0, 'F'},
                                           {"vcf", required_argument, 0, 'V'},
                                           {"samples", required_argument, 0, 'S'},
                                           {"ma-wsize", required_argument, 0, 'W'},
                                           {0, 0, 0, 0}};
    int c, long_index = 0;
    while ((c = getopt_long(argc, argv, "xo:k:lfsmha", long_options, &long_index)) != -1) {
        switch (c) {
            case 0: break;
            case 'x': args.fbb = 1; break;
            case 'o': args.prefix = optarg; break;
            case 's': args.tsa = 1; break;
            case 'm': args.ma = 1; break;
            case 'l': args.dl = 1; break;
            case 'f': args.ft = 1; break;
            case 'a': args.ft_only = 1; break;
            case 'k': args.k = std::strtoull(optarg, nullptr, 10); break;
            case 'G': args.device = atoi(optarg); break;
            case 'F': args.fasta = optarg; break;
            case 'V': args.vcf = optarg; break;
            case 'S': args.samples = optarg; args.has_samples = 1; break;
            case 'W': args.ma_wsize = std::strtoull(optarg, nullptr, 10); args.has_wsize = 1; break;
            case 'h': print_help(); exit(0);
            case '?': break;  // the reference ignores unknown options (rb_build.cpp:64-65)
            default: print_help(); exit(1);
        }
    }
    if (!args.vcf.empty() && (args.fasta.empty() || !args.ma)) {
        fprintf(stderr, "rb_build: --vcf needs --fasta and -m (it is the source of the marker array)\n");
        exit(1);
    }
    if (args.vcf.empty() && (args.has_samples || args.has_wsize)) {
        fprintf(stderr, "rb_build: --samples and --ma-wsize belong to --vcf\n");
        exit(1);
    }
    if (!args.fasta.empty()) {  // the input is the FASTA: no <index_prefix>, and the outputs need a name
        if (args.prefix.empty()) {
            fprintf(stderr, "rb_build: --fasta needs -o <output prefix>\n");
            exit(1);
        }
        args.inpre = args.prefix;
        return args;
    }
    if (argc - optind < 1) {
        fprintf(stderr, "no argument provided\n");
        exit(1);
    }
    args.inpre = argv[optind++];
    if (args.prefix.empty()) args.prefix = args.inpre;
    return args;
}

bool file_exists(const std::string &f) { return std::ifstream(f).good(); }

[[noreturn]] void die(const std::string &what, int rc) {
    std::cerr << "rb_build: " << what << ": " << rbg_strerror(rc) << std::endl;
    exit(1);
}

void file_ne_error(const std::string &f) {  // rowbowt_io.hpp:23-26
    std::cerr << f << " does not exist" << std::endl;
    exit(1);
}

void write_ftab(const Args &args) {
    rbg_index *ix = nullptr;
    int rc = rbg_load(args.prefix.c_str(), RBG_LOAD_NONE, args.device, &ix);  // .rbwt, else .rbgpu (rowbowt_io.hpp:127-139)
    if (rc == RBG_EIO) rc = rbg_build_from_files((args.inpre + ".bwt").c_str(), nullptr, nullptr, args.device, &ix);
    else if (!rc) std::cerr << "loading rbwt file" << std::endl;
    if (rc) die("loading the index for the ftab", rc);
    if ((rc = rbg_write_ftab(ix, args.k, (args.prefix + ".ftab").c_str()))) die("writing " + args.prefix + ".ftab", rc);
    rbg_free(ix);
}

// --fasta --vcf -m: the haplotype documents and their site records, the index and its marker array in one device build
int build_from_vcf(const Args &args) {
    if (args.ma_wsize < 1 || args.ma_wsize > 64) {
        std::cerr << "rb_build: --ma-wsize must be 1..64" << std::endl;
        return 1;
    }
    std::vector<std::string> samples;
    for (size_t a = 0; args.has_samples && a <= args.samples.size();) {
        size_t b = args.samples.find(',', a);
        if (b == std::string::npos) b = args.samples.size();
        samples.push_back(args.samples.substr(a, b - a));
        a = b + 1;
    }
    rbg_cli::VcfText v;
    std::string why;
    int rc = rbg_cli::vcf_text(args.fasta.c_str(), args.vcf.c_str(), args.has_samples ? &samples : nullptr, static_cast<uint32_t>(args.ma_wsize), v, &why);
    if (rc) {
        std::cerr << "rb_build: " << why << ": " << rbg_strerror(rc) << std::endl;
        return 1;
    }
    std::cerr << "skipped sites: " << v.skipped[rbg_cli::VCF_SKIP_INDEL] << " indel or MNV, " << v.skipped[rbg_cli::VCF_SKIP_SYMBOLIC] << " symbolic or non-ACGT, "
              << v.skipped[rbg_cli::VCF_SKIP_CONTIG] << " on a contig the FASTA lacks, " << v.skipped[rbg_cli::VCF_SKIP_DUPLICATE] << " duplicate position" << std::endl;
    for (const std::string &name : v.no_haplotypes)
        std::cerr << "rb_build: warning: sample " << name << " has no accepted site: its ploidy is unknown and it gets no documents" << std::endl;
    if (v.pos.empty()) {      // (-m was asked for: an index without a marker array is not what the caller wants)
        std::cerr << "rb_build: no site of " << args.vcf << " was accepted: there would be no marker array" << std::endl;
        return 1;
    }
    const std::string out = args.prefix + ".rbgpu", docs = v.t.docs_text();
    std::cerr << "constructing from " << args.fasta << " and " << args.vcf << ": " << v.t.names.size() << " documents, " << v.t.text.size() << " symbols, " << v.sites
              << " sites, " << v.pos.size() << " site records, windows of " << args.ma_wsize << std::endl;
    rc = rbg_convert_text_markers(reinterpret_cast<const uint8_t *>(v.t.text.data()), v.t.text.size(), v.pos.data(), v.first.data(), v.val.data(), v.pos.size(),
                                  static_cast<uint32_t>(args.ma_wsize), args.dl ? docs.c_str() : nullptr, args.tsa ? RBG_LOAD_SA : RBG_LOAD_NONE, args.device,
                                  out.c_str());
    if (rc) die("building " + out, rc);
    if (args.dl) {
        std::ofstream ofs(args.prefix + ".docs", std::ios::binary);
        ofs << docs;
        if (!ofs.good()) die("writing " + args.prefix + ".docs", RBG_EIO);
    }
    if (args.ft) write_ftab(args);
    return 0;
}

int build_from_fasta(const Args &args) {
    if (!args.vcf.empty()) return build_from_vcf(args);
    if (args.ma) {
        std::cerr << "rb_build: -m cannot be combined with --fasta: a FASTA carries no markers" << std::endl;
        return 1;
    }
    rbg_cli::FastaText t;
    std::string why;
    int rc = rbg_cli::fasta_text(args.fasta.c_str(), t, &why);
    if (rc) {
        std::cerr << "rb_build: " << why << ": " << rbg_strerror(rc) << std::endl;
        return 1;
    }
    const std::string out = args.prefix + ".rbgpu", docs = t.docs_text();
    std::cerr << "constructing from " << args.fasta << ": " << t.names.size() << " documents, " << t.text.size() << " symbols" << std::endl;
    rc = rbg_convert_text(reinterpret_cast<const uint8_t *>(t.text.data()), t.text.size(), args.dl ? docs.c_str() : nullptr, args.tsa ? RBG_LOAD_SA : RBG_LOAD_NONE,
                          args.device, out.c_str());
    if (rc) die("building " + out, rc);
    if (args.dl) {
        std::ofstream ofs(args.prefix + ".docs", std::ios::binary);
        ofs << docs;
        if (!ofs.good()) die("writing " + args.prefix + ".docs", RBG_EIO);
    }
    if (args.ft) write_ftab(args);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const Args args = parse_args(argc, argv);
    if (args.fbb) {
        std::cerr << "rb_build: fbb_string indexes are not supported by this engine" << std::endl;
        return 1;
    }
    if (!args.fasta.empty()) return build_from_fasta(args);
    if (args.ft_only) {  // rb_build.cpp:108-109
        write_ftab(args);
        return 0;
    }
    const std::string out = args.prefix + ".rbgpu";
    int rc;
    if (args.from_index) {
        int flags = RBG_LOAD_NONE;
        if (args.tsa) flags |= RBG_LOAD_SA;
        if (args.ma) flags |= RBG_LOAD_MA;
        if (args.dl) flags |= RBG_LOAD_DL;
        std::cerr << "converting " << args.inpre << ".rbwt to " << out << std::endl;
        if ((rc = rbg_convert_index(args.inpre.c_str(), flags, out.c_str()))) die("converting " + args.inpre, rc);
    } else {
        std::cerr << "constructing using rle_string (flat run-length BWT)" << std::endl;  // rowbowt_io.hpp:52
        const std::string bwt = args.inpre + ".bwt", ssa = args.inpre + ".ssa", esa = args.inpre + ".esa";
        const std::string mab = args.inpre + ".mab", docs = args.inpre + ".docs";
        if (!file_exists(bwt)) file_ne_error(bwt);
        if (args.tsa) {  // rowbowt_io.hpp:65-67
            if (!file_exists(ssa)) file_ne_error(ssa);
            if (!file_exists(esa)) file_ne_error(esa);
        }
        if (args.ma && !file_exists(mab)) {
            std::cerr << "rb_build: -m needs a serialised marker array " << mab
                      << " (the raw .ma reader belongs to pfbwt-f, which is not part of this engine)" << std::endl;
            return 1;
        }
        rc = rbg_convert_raw(bwt.c_str(), args.tsa ? ssa.c_str() : nullptr, args.tsa ? esa.c_str() : nullptr,
                             args.ma ? mab.c_str() : nullptr, (args.dl && file_exists(docs)) ? docs.c_str() : nullptr, out.c_str());
        if (rc) die("building " + out, rc);
        if (args.dl && docs != args.prefix + ".docs") {  // rowbowt_io.hpp:73-80: the .docs file is copied
            std::ifstream ifs(docs);
            std::ofstream ofs(args.prefix + ".docs");
            ofs << ifs.rdbuf();
        }
    }
    if (args.ft) write_ftab(args);  // rowbowt_io.hpp:82-88
    return 0;
}
