// Test harness (CPU only): the tools' read loop (rowbowt_amd/csrc/cli_pipeline.hpp) over a real InputSource with fake stages.
// usage: cli_pipeline_check <run|shards|throw|seq> <file> <window bytes> <batch> <threads>
//   run    run_pipeline: `query` copies every read's name and length into the slot (and sleeps 200 us, so that the stages
//          overlap), `format` prints "<name> <len>\n" per read through format_split.  stdout is the driver's own.
//   shards as run, but the text is made the ways rb_align --devices and rb_markers --device-format make it: batches with an
//          even ticket through format_ranges over three shards of the batch in format_threads slices each (3 T pieces in
//          (shard, slice) order; with fewer than three reads shards are empty, shard 0 among them), batches with an odd
//          ticket as one ready text through PiecePool::put.
//   throw  as run, but `format` throws on batch 3 of window 2 (both counted from 0): the driver must rethrow once the
//          query ahead, the scanner and the writer have returned; stdout then holds windows 0 and 1.
//   seq    run_in_sequence: the driver writes nothing; the lines that `query` collected are printed after it has returned.
// The call order is checked here as the stages run (a violation: "CHECK FAILED: ..." on stderr, exit 3):
//   on_window once per window, on the main thread, before the window's first prepare, after the previous window's last batch;
//   prepare on the main thread, batches in file order, each before its own query; the ticket it draws is the one `format`
//   finds in the slot (as rb_markers' coins are drawn); query of batch 0 of a window on the main thread, of every other batch
//   on another thread, started before the format of the batch before it ends; format on the main thread, only of a slot
//   whose query has returned; seq: prepare and query alternate strictly, slot 0.
// stderr, last line before an input error's message:
//   "rc=<code> windows=<n> window_sizes=<a,b,...> batches=<n> ahead=<n> pieces_held=<n> max_window_pieces=<n>"
// (ahead: queries that ran off the main thread).  The run ends through exit_on_input_error like the tools: exit 1 with
// kseq's message for -2 / -3.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "../../rowbowt_amd/csrc/cli_pipeline.hpp"

namespace {

using rbg_cli::BatchView;
using rbg_cli::PiecePool;
using rbg_cli::TextBuf;
using rbg_cli::Window;

[[noreturn]] void fail(const char *what) {
    std::fprintf(stderr, "CHECK FAILED: %s\n", what);
    _exit(3);
}
void check(bool ok, const char *what) {
    if (!ok) fail(what);
}

struct Slot {
    long ticket = -1;        // drawn in prepare
    long queried = -1;       // the ticket whose query has returned
    size_t w0 = 0, n = 0;    // the batch's bounds as prepare saw them
    std::vector<std::string> names;
    std::vector<uint64_t> lens;
};

struct Stages {
    const std::thread::id main_thread = std::this_thread::get_id();
    size_t batch = 1, threads = 1;
    Slot slots[2];
    long next_ticket = 0, next_format = 0;
    std::atomic<long> started{-1};   // the highest ticket whose query has begun
    std::vector<size_t> window_sizes;
    size_t next_w0 = 0;              // where the next batch of the window must begin
    size_t window_pieces = 0, max_window_pieces = 0;
    std::atomic<size_t> ahead_count{0};
    bool sequential = false, prepared_not_queried = false, shards = false;
    long throw_window = -1, throw_batch = -1;
    std::string collected;           // seq: the lines, printed after the driver has returned

    void on_window(const Window &w) {
        check(std::this_thread::get_id() == main_thread, "on_window off the main thread");
        check(window_sizes.empty() || next_w0 == window_sizes.back(), "on_window before the previous window's last batch");
        window_sizes.push_back(w.size());
        next_w0 = 0;
        window_pieces = 0;
    }
    void prepare(const BatchView &b, size_t s) {
        check(std::this_thread::get_id() == main_thread, "prepare off the main thread");
        check(!window_sizes.empty() && b.w->size() == window_sizes.back(), "prepare before its window's on_window");
        check(b.w0 == next_w0 && b.n >= 1 && b.n == std::min(batch, b.w->size() - b.w0), "prepare out of file order");
        check(s == (sequential ? size_t(0) : (b.w0 / batch) & 1), "slot index");
        check(!prepared_not_queried, "two prepares without a query between them");
        if (sequential) prepared_not_queried = true;
        next_w0 += b.n;
        Slot &slot = slots[s];
        check(slot.queried == slot.ticket, "prepare of a slot whose query is still running");
        slot.ticket = next_ticket++;
        slot.w0 = b.w0;
        slot.n = b.n;
    }
    void query(const BatchView &b, size_t s) {
        Slot &slot = slots[s];
        check(slot.ticket >= 0 && slot.w0 == b.w0 && slot.n == b.n && slot.queried != slot.ticket, "query without its prepare");
        const bool on_main = std::this_thread::get_id() == main_thread;
        check(on_main == (sequential || b.w0 == 0), "query on the wrong thread");
        if (!on_main) ahead_count.fetch_add(1);
        started.store(slot.ticket);
        slot.names.clear();
        slot.lens.clear();
        for (size_t i = 0; i < b.size(); ++i) {
            slot.names.emplace_back(b.name(i), b.name_len(i));
            slot.lens.push_back(b.seq_len(i));
        }
        if (sequential) {
            check(prepared_not_queried, "query without a prepare right before it");
            prepared_not_queried = false;
            for (size_t i = 0; i < b.size(); ++i) collected += slot.names[i] + " " + std::to_string(slot.lens[i]) + "\n";
        } else {
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
        slot.queried = slot.ticket;
    }
    void format(const BatchView &b, size_t s, PiecePool &pool) {
        check(std::this_thread::get_id() == main_thread, "format off the main thread");
        Slot &slot = slots[s];
        check(slot.ticket == next_format && slot.queried == slot.ticket, "format of a slot whose query has not returned");
        check(slot.w0 == b.w0 && slot.n == b.n && slot.names.size() == b.n, "format of another batch than the slot's");
        ++next_format;
        if (static_cast<long>(window_sizes.size()) - 1 == throw_window && static_cast<long>(b.w0 / batch) == throw_batch)
            throw std::runtime_error("format failed");
        auto write_lines = [&](size_t i0, size_t i1, TextBuf &piece) {
            rbg_cli::FastOut out(piece);
            for (size_t i = i0; i < i1; ++i) {
                char *p = out.room(slot.names[i].size() + 32);
                char *const p0 = p;
                p = rbg_cli::fmt_lit(p, slot.names[i].data(), slot.names[i].size());
                *p++ = ' ';
                p = rbg_cli::fmt_u64(p, slot.lens[i]);
                *p++ = '\n';
                out.len += static_cast<size_t>(p - p0);
            }
            out.finish();
        };
        const size_t T = rbg_cli::format_threads(b.n, threads), G = 3;
        window_pieces += !shards ? T : (slot.ticket & 1) ? 1 : G * T;
        max_window_pieces = std::max(max_window_pieces, window_pieces);
        if (!shards) {
            rbg_cli::format_split(b.n, threads, pool, write_lines);
        } else if (slot.ticket & 1) {
            TextBuf whole;
            write_lines(0, b.n, whole);
            pool.put(whole.data(), whole.size());
        } else {
            std::vector<std::pair<size_t, size_t>> ranges;
            for (size_t g = 0; g < G; ++g) rbg_cli::add_slices(b.n * g / G, b.n * (g + 1) / G - b.n * g / G, T, ranges);
            check(ranges.size() == G * T, "pieces of a sharded batch");
            rbg_cli::format_ranges(ranges, pool, [&](size_t k, size_t i0, size_t i1, TextBuf &piece) {
                check(k / T < G && i0 >= b.n * (k / T) / G && i1 <= b.n * (k / T + 1) / G, "a slice outside its shard");
                check(k == 0 || i0 < i1, "an empty slice on a thread of its own");
                write_lines(i0, i1, piece);
            });
        }
        // the next batch's query was started before this format: it begins while this one is still here (a driver that
        // ran the stages one after the other would never get past this wait)
        if (b.w0 + b.n < b.w->size())
            for (int spins = 0; started.load() < slot.ticket + 1; ++spins) {
                check(spins < 50000, "the next batch's query did not start during this format");
                std::this_thread::sleep_for(std::chrono::microseconds(100));
            }
    }
};

}  // namespace

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    const std::string mode = argv[1];
    rbg_cli::InputSource in;
    Stages st;
    st.batch = std::max<size_t>(1, std::strtoull(argv[4], nullptr, 10));
    st.threads = std::max<size_t>(1, std::strtoull(argv[5], nullptr, 10));
    if (!in.open(argv[2], static_cast<unsigned>(st.threads), std::strtoull(argv[3], nullptr, 10), 1)) {
        std::fprintf(stderr, "invalid file\n");
        return 2;
    }
    auto on_window = [&](const Window &w) { st.on_window(w); };
    auto prepare = [&](const BatchView &b, size_t s) { st.prepare(b, s); };
    auto query = [&](const BatchView &b, size_t s) { st.query(b, s); };
    auto format = [&](const BatchView &b, size_t s, PiecePool &pool) { st.format(b, s, pool); };
    rbg_cli::PipelineBuffers bufs;
    int rc = 0;
    st.shards = mode == "shards";
    if (mode == "seq") {
        st.sequential = true;
        rc = rbg_cli::run_in_sequence(in, st.batch, bufs, on_window, prepare, query);
        check(!st.prepared_not_queried, "a prepare without its query");
        std::fwrite(st.collected.data(), 1, st.collected.size(), stdout);
    } else if (mode == "throw") {
        st.throw_window = 2;
        st.throw_batch = 3;
        try {
            rc = rbg_cli::run_pipeline(in, st.batch, bufs, on_window, prepare, query, format);
            fail("format threw nothing: the input has no batch 3 in window 2");
        } catch (const std::runtime_error &) {
            // every thread of the driver has returned: the slots, the input and stdout are this thread's alone again
            for (Slot &slot : st.slots) check(slot.queried == slot.ticket, "a query was still running when the exception left the driver");
            (void)in.next(bufs.nxt);
        }
    } else {
        rbg_cli::PipelineStats waits;
        rc = rbg_cli::run_pipeline(in, st.batch, bufs, on_window, prepare, query, format, &waits);
        check(waits.scan_wait_s >= 0 && waits.write_wait_s >= 0, "waits");
    }
    std::fflush(stdout);
    const size_t pieces_held = std::max(bufs.pool.pieces.size(), bufs.writing.pieces.size());
    check(pieces_held <= st.max_window_pieces, "a pool holds more pieces than the largest window needed");
    std::string sizes;
    for (size_t v : st.window_sizes) sizes += (sizes.empty() ? "" : ",") + std::to_string(v);
    std::fprintf(stderr, "rc=%d windows=%zu window_sizes=%s batches=%ld ahead=%zu pieces_held=%zu max_window_pieces=%zu\n", rc, st.window_sizes.size(),
                 sizes.c_str(), st.next_ticket, st.ahead_count.load(), pieces_held, st.max_window_pieces);
    rbg_cli::exit_on_input_error(rc);
    return 0;
}
