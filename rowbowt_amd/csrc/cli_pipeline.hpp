// cli_pipeline.hpp -- the read loop shared by the command-line tools (rb_align, rb_markers, rb_locs): the input window by
// window (cli_input.hpp), every window in batches of --batch reads, the text in a recycled pool of pieces (fastx.hpp).
// Three overlapped stages: scan window i+1 | query + format window i | write window i-1; inside a window batch j+1 is
// queried while batch j is formatted.  What a tool does with a batch -- its slot type, its library calls, its text --
// stays in the tool and comes in as callables.  Host C++17, nothing of HIP or rbg.h: tests/cpp/cli_pipeline_check.cpp
// runs it with fake stages under the sanitizers.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "cli_input.hpp"
#include "fastx.hpp"

namespace rbg_cli {

// reads [w0, w0 + n) of a window, where the scanner found them (names and sequences are spans of the window's buffer)
struct BatchView {
    const Window *w;
    size_t w0, n;
    size_t size() const { return n; }
    const char *name(size_t i) const { return w->base + w->recs.name_begin[w0 + i]; }
    size_t name_len(size_t i) const { return w->recs.name_len[w0 + i]; }
    const char *seq(size_t i) const { return w->base + w->recs.seq_begin[w0 + i]; }
    uint64_t seq_len(size_t i) const { return w->recs.seq_len[w0 + i]; }
    // the quality string of record i (seq_len(i) bytes), or nullptr for a FASTA record
    const char *qual(size_t i) const { const uint64_t q = w->recs.qual_begin[w0 + i]; return q == RecordSpans::kNoQual ? nullptr : w->base + q; }
    bool all_have_qual() const {
        for (size_t i = 0; i < n; ++i)
            if (w->recs.qual_begin[w0 + i] == RecordSpans::kNoQual) return false;
        return true;
    }
};

// the raw reads of a batch back to back: read i is seqs[off[i] .. off[i + 1])
inline void pack_raw_reads(const BatchView &b, std::string &seqs, std::vector<uint64_t> &off) {
    const size_t N = b.size();
    off.resize(N + 1);
    off[0] = 0;
    for (size_t i = 0; i < N; ++i) off[i + 1] = off[i] + b.seq_len(i);
    seqs.resize(off[N]);
    for (size_t i = 0; i < N; ++i) std::memcpy(&seqs[off[i]], b.seq(i), b.seq_len(i));
}

// The text of one window, as pieces in output order.  The pool keeps its buffers -- and their pages -- from window to
// window: `used` counts the ones of this window (fresh 12 MB buffers per batch cost more in page faults than the
// formatting itself).
struct PiecePool {
    std::vector<TextBuf> pieces;
    size_t used = 0;
    // the next n pieces, cleared.  The pointer holds until the next take() or put(), which may grow the vector: take what
    // a batch needs in one call and finish with it before the next.
    TextBuf *take(size_t n) {
        const size_t first = used;
        used += n;
        if (pieces.size() < used) pieces.resize(used);
        for (size_t i = first; i < used; ++i) pieces[i].clear();
        return pieces.data() + first;
    }
    // a text made elsewhere (on the device) as the next piece
    void put(const char *text, size_t len) {
        TextBuf &piece = *take(1);
        piece.reserve(len);
        if (len) std::memcpy(piece.p.get(), text, len);
        piece.len = len;
    }
    void write(FILE *f) const {
        for (size_t i = 0; i < used; ++i)
            if (pieces[i].size()) fwrite(pieces[i].data(), 1, pieces[i].size(), f);   // (the piece of an empty slice may never have had a buffer)
    }
};

// formatting workers for N reads: a slice is worth a thread from 4096 reads on
inline size_t format_threads(size_t N, size_t threads) { return std::max<size_t>(1, std::min<size_t>({threads, (N + 4095) / 4096, size_t(64)})); }

// One piece per range, in the ranges' order: fn(k, i0, i1, piece) for range k = [i0, i1).  Range 0 runs on the caller's
// thread, every other non-empty range on a thread of its own, all of them at once.  The pieces are taken once, before any
// fn runs: fn writes its piece and must not take or put pieces itself (take() may move the ones handed out before it).
template <class Fn>
void format_ranges(const std::vector<std::pair<size_t, size_t>> &ranges, PiecePool &pool, Fn fn) {
    if (ranges.empty()) return;
    TextBuf *piece = pool.take(ranges.size());
    std::vector<std::thread> workers;
    for (size_t k = 1; k < ranges.size(); ++k)
        if (ranges[k].first != ranges[k].second) workers.emplace_back([&ranges, &fn, piece, k] { fn(k, ranges[k].first, ranges[k].second, piece[k]); });
    fn(size_t(0), ranges[0].first, ranges[0].second, piece[0]);
    for (auto &w : workers) w.join();
}
// the slices [begin + n * t / T, begin + n * (t + 1) / T) of n reads, appended to `ranges`
inline void add_slices(size_t begin, size_t n, size_t T, std::vector<std::pair<size_t, size_t>> &ranges) {
    for (size_t t = 0; t < T; ++t) ranges.emplace_back(begin + n * t / T, begin + n * (t + 1) / T);
}
// reads [0, N) in format_threads(N, threads) slices: fn(i0, i1, piece)
template <class Fn>
void format_split(size_t N, size_t threads, PiecePool &pool, Fn fn) {
    std::vector<std::pair<size_t, size_t>> ranges;
    add_slices(0, N, format_threads(N, threads), ranges);
    format_ranges(ranges, pool, [&fn](size_t, size_t i0, size_t i1, TextBuf &piece) { fn(i0, i1, piece); });
}

// for a stage that a tool does not have
struct NoStage {
    template <class... A>
    void operator()(A &&...) const {}
};
constexpr NoStage no_stage{};

struct PipelineStats {
    double scan_wait_s = 0, write_wait_s = 0;   // seconds the main thread waited for the scanner and for the writer
};

// What the loop keeps from window to window: the window being worked on and the one being scanned, the pool being filled and
// the one being written.  It lives in the tool's main(), beyond its timers: giving some hundred MB of records and text back
// to the system takes milliseconds that are not the loop's.
struct PipelineBuffers {
    Window cur, nxt;
    PiecePool pool, writing;
};

// The windows of the input in file order: window i+1 is scanned on a thread of its own while body(window i) runs.  Returns
// the scanner's final code (InputSource::next: -1 at the end of the input, -2 / -3 like kseq_read).  An exception from
// `body` leaves once the scanner has returned.
template <class Body>
int for_each_window(InputSource &input, Window &cur, Window &nxt, Body body, double *scan_wait_s = nullptr) {
    int err = input.next(cur);
    while (true) {
        std::future<int> scanner;
        const bool more = err == 0;
        if (more) scanner = std::async(std::launch::async, [&input, &nxt] { return input.next(nxt); });
        body(cur);
        if (!more) break;
        const auto t0 = std::chrono::steady_clock::now();
        err = scanner.get();
        if (scan_wait_s) *scan_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::swap(cur, nxt);
    }
    return err;
}

inline size_t batches_of(const Window &w, size_t batch) { return (w.size() + batch - 1) / batch; }
inline BatchView batch_view(const Window &w, size_t batch, size_t j) { return BatchView{&w, j * batch, std::min<size_t>(w.size() - j * batch, batch)}; }

// The tools' loop.  All callables run on the main thread unless said otherwise; `slot` is j & 1 for batch j of a window
// (the slot objects are the tool's).
//   on_window(const Window &)         before the window's first batch
//   prepare(BatchView, slot)          in file order, immediately before that batch's query is started
//   query(BatchView, slot)            batch 0 of a window on the main thread, batch j+1 on a thread of its own while batch j is formatted
//   format(BatchView, slot, pool)     after the batch's query has returned; may throw
// A window's pieces are written to stdout behind the loop while the next window is worked on.  An exception from `format`
// leaves once the query ahead, the scanner and the writer have returned (the futures join while unwinding); the failed
// window's text is dropped.  Returns for_each_window's code; the caller flushes stdout.
template <class OnWindow, class Prepare, class Query, class Format>
int run_pipeline(InputSource &input, size_t batch, PipelineBuffers &bufs, OnWindow on_window, Prepare prepare, Query query, Format format,
                 PipelineStats *stats = nullptr) {
    PipelineStats st;
    PiecePool &pool = bufs.pool, &writing = bufs.writing;
    std::future<void> writer;
    const int err = for_each_window(input, bufs.cur, bufs.nxt, [&](const Window &cur) {
        pool.used = 0;
        on_window(cur);
        {
            const size_t nb = batches_of(cur, batch);
            std::future<void> ahead;
            if (nb) {
                prepare(batch_view(cur, batch, 0), size_t(0));
                query(batch_view(cur, batch, 0), size_t(0));
            }
            for (size_t j = 0; j < nb; ++j) {
                if (ahead.valid()) ahead.get();
                if (j + 1 < nb) {
                    const BatchView nv = batch_view(cur, batch, j + 1);
                    const size_t ns = (j + 1) & 1;
                    prepare(nv, ns);
                    ahead = std::async(std::launch::async, [&query, nv, ns] { query(nv, ns); });
                }
                format(batch_view(cur, batch, j), j & 1, pool);
            }
        }
        const auto t0 = std::chrono::steady_clock::now();
        if (writer.valid()) writer.get();
        st.write_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::swap(pool, writing);
        writer = std::async(std::launch::async, [&writing] { writing.write(stdout); });
    }, &st.scan_wait_s);
    if (writer.valid()) writer.get();
    if (stats) *stats = st;
    return err;
}

// The loop without look-ahead and without text (rb_markers --tally): per batch prepare, then query, in sequence on the
// main thread, always with slot 0.
template <class OnWindow, class Prepare, class Query>
int run_in_sequence(InputSource &input, size_t batch, PipelineBuffers &bufs, OnWindow on_window, Prepare prepare, Query query) {
    return for_each_window(input, bufs.cur, bufs.nxt, [&](const Window &cur) {
        on_window(cur);
        for (size_t j = 0; j < batches_of(cur, batch); ++j) {
            prepare(batch_view(cur, batch, j), size_t(0));
            query(batch_view(cur, batch, j), size_t(0));
        }
    });
}

// what kseq_read's error codes end a tool with (rb_align.cpp:182-191)
inline void exit_on_input_error(int err) {
    switch (err) {
        case -2: fprintf(stderr, "ERROR: truncated quality string\n"); exit(1);
        case -3: fprintf(stderr, "ERROR: error reading stream\n"); exit(1);
        default: break;
    }
}

}  // namespace rbg_cli
