// rb_locs -- drop-in for the reference's second genotyping tool (reference src/rb_markers_tsa.cpp, built as rb_locs)
//   rb_locs [-w wsize] [-m max_hits] [-o prefix] <index_prefix> <fastq>
// For every read: the locations of its longest greedy seed (find_locs_greedy_seeding(seq, wsize, max_hits), rb_markers_tsa.cpp:78), and for
// every location l the markers of <index_prefix>.midx -- a marker index keyed by TEXT position -- that overlap [l, l + len - 1] (:82).  The
// per-read loop of the reference becomes one batched call into the MI355X engine (rbg_find_loc_markers_greedy_seeding, include/rbg.h): the
// locations never leave the device between the locate and the marker lookup.
//
// One stdout line per read (:79-87):  "<name>" { " <seq>/<pos>/<allele>" } "\n"  -- the markers location after location, unsorted and with
// repeats, as the reference prints them; a read without locations or markers prints its name alone.  The read is searched as it stands in the
// file (no nt table, no reverse complement: :78 passes seq->seq.s).
//
// The index is loaded with SA | DL like the reference (:90-95: a missing .tsa or .docs exits 1), although resolve_offset's result (:81) is
// never printed.  -o is accepted and unused, as there.
#include <getopt.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <string>
#include <thread>
#include <vector>

#include "../include/rowbowt_gpu.hpp"
#include "fastx.hpp"
#include "cli_input.hpp"
#include "cli_pipeline.hpp"

namespace {

using rbg_cli::InputSource;
using rbg_cli::BatchView;

struct RbLocsArgs {  // rb_markers_tsa.cpp:14-20
    std::string inpre, fastq_fname, outpre;
    uint64_t max_hits = ~uint64_t(0);
    uint64_t wsize = 10;
    uint64_t threads = 8;
    int device = 0;
    uint64_t batch = 1u << 18;
};

void print_help() {  // rb_markers_tsa.cpp:22-28
    fprintf(stderr, "rb_locs_only");
    fprintf(stderr, "Usage: rb_locs_only [options] <index_prefix> <input_fastq_name>\n");
    fprintf(stderr, "    --wsize/-w         <int>         minimum seed length (default 10)\n");
    fprintf(stderr, "    --max-hits/-m      <int>         locations per read at most (default: all)\n");
    fprintf(stderr, "    --output_prefix/-o <basename>    output prefix\n");
    fprintf(stderr, "    --gpu <n>                        HIP device ordinal (default 0)\n");
    fprintf(stderr, "    --batch <n>                      reads per GPU batch (default 262144)\n");
    fprintf(stderr, "    <input_prefix>                   index prefix\n");
    fprintf(stderr, "    <input_fastq>                    input fastq\n");
}

RbLocsArgs parse_args(int argc, char **argv) {  // rb_markers_tsa.cpp:30-73
    RbLocsArgs args;
    static struct option long_options[] = {{"wsize", required_argument, 0, 'w'},
                                           {"output_prefix", required_argument, 0, 'o'},
                                           {"max-hits", required_argument, 0, 'm'},
                                           {"threads", required_argument, 0, 't'},
                                           {"gpu", required_argument, 0, 'G'},
                                           {"batch", required_argument, 0, 'B'},
                                           {0, 0, 0, 0}};
    int c, long_index = 0;
    while ((c = getopt_long(argc, argv, "o:w:m:h", long_options, &long_index)) != -1) {
        switch (c) {
            case 'w': args.wsize = static_cast<uint64_t>(std::atol(optarg)); break;
            case 'm': args.max_hits = static_cast<uint64_t>(std::atol(optarg)); break;
            case 'o': args.outpre = optarg; break;
            case 't': args.threads = static_cast<uint64_t>(std::atol(optarg)); break;
            case 'G': args.device = atoi(optarg); break;
            case 'B': args.batch = strtoull(optarg, nullptr, 10); break;
            case 'h': print_help(); exit(0);
            default: print_help(); exit(1);
        }
    }
    if (argc - optind < 2) {
        fprintf(stderr, "no argument provided\n");
        exit(1);
    }
    args.inpre = argv[optind++];
    args.fastq_fname = argv[optind++];
    if (args.outpre.empty()) args.outpre = args.inpre;
    if (args.batch == 0) args.batch = 1;
    if (args.threads == 0) args.threads = 1;
    return args;
}

// One batch between the two stages of the loop: the library call | markers -> text
struct LocSlot {
    std::string seqs;
    std::vector<uint64_t> off, loc_off, mk_off;
    uint64_t *locs = nullptr, *mk = nullptr;
    int rc = RBG_OK;
    double t_query = 0;
    ~LocSlot() { rbg_free_buffer(locs); rbg_free_buffer(mk); }
};

double g_trace[2] = {0, 0};   // RB_ALIGN_TRACE=1: seconds in the library call, formatting

// stage 1: the reads' bytes as they are, one library call
void query_batch(const rbwt::RowBowt<> &rb, const RbLocsArgs &args, const BatchView &b, LocSlot &slot) {
    const size_t N = b.size();
    const auto t0 = std::chrono::steady_clock::now();
    rbg_cli::pack_raw_reads(b, slot.seqs, slot.off);
    rbg_free_buffer(slot.locs);
    rbg_free_buffer(slot.mk);
    slot.locs = slot.mk = nullptr;
    slot.loc_off.resize(N + 1);
    slot.mk_off.resize(N + 1);
    slot.rc = rbg_find_loc_markers_greedy_seeding(rb.handle(), reinterpret_cast<const uint8_t *>(slot.seqs.data()), slot.off.data(), N, args.wsize,
                                                  args.max_hits, slot.loc_off.data(), &slot.locs, slot.mk_off.data(), &slot.mk);
    slot.t_query = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// text for reads [i0, i1) (rb_report, rb_markers_tsa.cpp:79-87)
void format_range(const BatchView &b, const LocSlot &r, size_t i0, size_t i1, rbg_cli::TextBuf &out_s) {
    using rbg_cli::fmt_lit;
    using rbg_cli::fmt_u64;
    rbg_cli::FastOut out(out_s);
    for (size_t i = i0; i < i1; ++i) {
        const size_t name_len = b.name_len(i);
        const uint64_t m0 = r.mk_off[i], m1 = r.mk_off[i + 1];
        char *p = out.room(name_len + 2 + (m1 - m0) * 64);
        char *const p0 = p;
        p = fmt_lit(p, b.name(i), name_len);
        for (uint64_t t = m0; t < m1; ++t) {
            const MarkerT m = r.mk[t];
            *p++ = ' ';
            p = fmt_u64(p, get_seq(m));
            *p++ = '/';
            p = fmt_u64(p, get_pos(m));
            *p++ = '/';
            p = fmt_u64(p, static_cast<uint64_t>(get_allele(m)));
        }
        *p++ = '\n';
        out.len += static_cast<size_t>(p - p0);
    }
    out.finish();
}

// stage 2
void format_batch(const RbLocsArgs &args, const BatchView &b, LocSlot &slot, rbg_cli::PiecePool &pool) {
    rbwt::detail::check(slot.rc, "rbg_find_loc_markers_greedy_seeding");
    const auto t0 = std::chrono::steady_clock::now();
    rbg_cli::format_split(b.size(), static_cast<size_t>(args.threads), pool, [&](size_t i0, size_t i1, rbg_cli::TextBuf &piece) { format_range(b, slot, i0, i1, piece); });
    g_trace[0] += slot.t_query;
    g_trace[1] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

bool readable(const std::string &fname) {
    FILE *f = std::fopen(fname.c_str(), "rb");
    if (!f) return false;
    std::fclose(f);
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    const RbLocsArgs args = parse_args(argc, argv);
    auto start = std::chrono::high_resolution_clock::now();
    rbwt::RowBowt<> rb = rbwt::load_rowbowt<>(args.inpre, rbwt::LoadRbwtFlag::DL | rbwt::LoadRbwtFlag::SA, args.device);  // rb_markers_tsa.cpp:90-95
    // :99-101 (the reference reads from a stream it never checks; a missing marker index can only be a mistake)
    const std::string midx = args.inpre + ".midx";
    if (!readable(midx)) {
        fprintf(stderr, "rb_locs: cannot read the marker index %s\n", midx.c_str());
        exit(1);
    }
    rb.load_text_markers(midx);
    std::chrono::duration<double> diff = std::chrono::high_resolution_clock::now() - start;
    std::cerr << "loading rowbowt + marker index took: " << diff.count() << " seconds\n";

    start = std::chrono::high_resolution_clock::now();
    InputSource input;  // :103-108 (plain, gzip or a pipe; scanned in place, window by window: cli_input.hpp)
    if (!input.open(args.fastq_fname, static_cast<unsigned>(std::max<uint64_t>(1, args.threads)), uint64_t(256) << 20)) {
        fprintf(stderr, "invalid file\n");
        exit(1);
    }
    // the shared loop (cli_pipeline.hpp): batch j + 1 is searched while batch j is printed
    LocSlot slots[2];
    rbg_cli::PipelineBuffers bufs;
    const int err = rbg_cli::run_pipeline(
        input, args.batch, bufs, rbg_cli::no_stage, rbg_cli::no_stage, [&](const BatchView &b, size_t s) { query_batch(rb, args, b, slots[s]); },
        [&](const BatchView &b, size_t s, rbg_cli::PiecePool &pool) { format_batch(args, b, slots[s], pool); });
    fflush(stdout);
    rbg_cli::exit_on_input_error(err);  // rb_markers_tsa.cpp:114-123
    diff = std::chrono::high_resolution_clock::now() - start;
    if (std::getenv("RB_ALIGN_TRACE")) fprintf(stderr, "rb_locs loop: library call %.3f s, markers -> text %.3f s\n", g_trace[0], g_trace[1]);
    std::cerr << "locating markers took: " << diff.count() << " seconds" << std::endl;
    return 0;
}
