// rowbowt_gpu.hpp -- source-compatible stand-in for the reference's query API on top of the
// C-ABI (include/rbg.h).  A caller written against
//     rbwt::load_rowbowt<StringT>(prefix, flag)            include/rowbowt_io.hpp:176-189
//     rbwt::RowBowt<StringT>::find_range / count / find_range_w_toehold / locs_at /
//         markers_at / find_range_w_markers / resolve_offset / LF / full_range / get_f
//                                                          include/rowbowt.hpp
// compiles against this header unchanged (swap the two #includes) and gets bit-identical
// answers, computed on an MI355X.  Per-read calls cost a kernel launch each, so the class also
// offers *_batch forms; rb_align (rowbowt_amd/csrc/rb_align.cpp) uses those.
//
// Error behaviour follows the reference: a missing file prints to stderr and exit(1)s
// (rowbowt_io.hpp:166-169); a query on a structure that was not loaded returns the default value
// (rowbowt.hpp:171, :273, :294-297); a failed search is in-band {1,0}.  Anything the reference
// would not survive (no GPU, HIP failure) also goes to stderr + exit(1).
//
// Also offered (next-row f4): find_locs_greedy_seeding, get_markers_greedy_seeding (with and without
// a loaded ftab), get_markers_lmems (with a loaded ftab, as in the reference).  Not implemented here: overlap seeding
// (the reference refuses it itself).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rbg.h"
#include "../csrc/rbg_docdir.hpp"   // the document lookup rule, stated once for library, kernels and this header

// pfbwt-f marker_array.hpp helpers used at rb_align.cpp:142 (bit layout: SURVEY.md 8b-format)
using MarkerT = uint64_t;
inline uint64_t get_pos(MarkerT m) { return m & ((uint64_t(1) << 48) - 1); }
inline uint64_t get_seq(MarkerT m) { return (m >> 48) & 0xFFF; }
inline uint8_t get_allele(MarkerT m) { return static_cast<uint8_t>((m >> 60) & 0xF); }

namespace ri {
struct rle_string_sd {};  // tag only: keeps `RowBowt<ri::rle_string_sd>` spelling valid
}

namespace rbwt {

using rle_string_t = ri::rle_string_sd;

// rowbowt_io.hpp:146-158
enum class LoadRbwtFlag { NONE = 0, SA = 1, MA = 2, DL = 4, FT = 8 };
inline constexpr LoadRbwtFlag operator|(LoadRbwtFlag a, LoadRbwtFlag b) {
    return static_cast<LoadRbwtFlag>(static_cast<int>(a) | static_cast<int>(b));
}
inline constexpr LoadRbwtFlag operator&(LoadRbwtFlag a, LoadRbwtFlag b) {
    return static_cast<LoadRbwtFlag>(static_cast<int>(a) & static_cast<int>(b));
}

namespace detail {
[[noreturn]] inline void die(const char *what, int rc) {
    std::cerr << what << ": " << rbg_strerror(rc) << std::endl;
    std::exit(1);
}
inline void check(int rc, const char *what) {
    if (rc != RBG_OK) die(what, rc);
}
struct Batch {  // reads -> the C-ABI's (seqs, off) layout
    std::string seqs;
    std::vector<uint64_t> off{0};
    void add(const std::string &s) { seqs += s; off.push_back(seqs.size()); }
    const uint8_t *data() const { return reinterpret_cast<const uint8_t *>(seqs.data()); }
    uint64_t size() const { return off.size() - 1; }
};
struct LibBuf {  // library-malloc'ed ragged output
    uint64_t *p = nullptr;
    ~LibBuf() { rbg_free_buffer(p); }
};
}  // namespace detail

// The marker tally of an index (include/rbg.h, rbg_tally_*): per marker, how many of rb_markers' lines carried it, accumulated on the device by
// RowBowt::markers_tally.  Destroy it before the RowBowt it was made from; feed it from one thread at a time.
class MarkerTally {
   public:
    MarkerTally() {}
    MarkerTally(rbg_index *ix, uint64_t distinct_hint) {
        rbg_tally *t = nullptr;
        detail::check(rbg_tally_create(ix, distinct_hint, &t), "rbg_tally_create");
        t_.reset(t);
    }
    rbg_tally *handle() const { return t_.get(); }
    void reset() { detail::check(rbg_tally_reset(t_.get()), "rbg_tally_reset"); }
    void reserve(uint64_t extra) { detail::check(rbg_tally_reserve(t_.get(), extra), "rbg_tally_reserve"); }
    void add_entries(const std::vector<rbg_tally_entry_t> &entries) {
        detail::check(rbg_tally_add_entries(t_.get(), entries.data(), entries.size()), "rbg_tally_add_entries");
    }
    // the entries with n_fwd + n_rev > 0, sorted by (sequence, position, allele)
    std::vector<rbg_tally_entry_t> entries() const {
        uint64_t n = 0;
        rbg_tally_entry_t *p = nullptr;
        detail::check(rbg_tally_export(t_.get(), &n, &p), "rbg_tally_export");
        std::unique_ptr<rbg_tally_entry_t, void (*)(void *)> hold(p, rbg_free_buffer);
        return std::vector<rbg_tally_entry_t>(p, p + n);
    }
    struct Info { uint64_t entries, capacity, grows, records, elements, dropped; };
    Info info() const {
        uint64_t v[6];
        detail::check(rbg_tally_info(t_.get(), v), "rbg_tally_info");
        return Info{v[0], v[1], v[2], v[3], v[4], v[5]};
    }
    // what the per-read adds (markers_tally with RBG_TALLY_PER_READ) saw: elements_seen = the elements they added + lost + site_dropped
    struct ReadInfo { uint64_t reads, elements_seen, lost, site_dropped; };
    ReadInfo read_info() const {
        uint64_t v[4];
        detail::check(rbg_tally_read_info(t_.get(), v), "rbg_tally_read_info");
        return ReadInfo{v[0], v[1], v[2], v[3]};
    }

   private:
    struct Free { void operator()(rbg_tally *t) const { rbg_tally_free(t); } };
    std::unique_ptr<rbg_tally, Free> t_;
};

template <typename RLEString = rle_string_t>
class RowBowt {
   public:
    using range_t = std::pair<uint64_t, uint64_t>;

    // rowbowt.hpp:133-165
    struct LFData {
        LFData() {}
        LFData(range_t r, uint64_t s, uint64_t e, uint64_t ss) : rn(r), qstart(s), qend(e), ssamp(ss) {}
        LFData(range_t r, uint64_t s, uint64_t e) : rn(r), qstart(s), qend(e) {}  // (:148-152 leaves ssamp unset; 0 here)
        void clear() { rn = {1, 0}; qstart = 0; qend = 0; ssamp = 0; markers.clear(); }
        range_t rn = {1, 0};
        uint64_t qstart = 0;
        uint64_t qend = 0;
        uint64_t ssamp = 0;
        std::vector<MarkerT> markers;
    };

    RowBowt() {}
    explicit RowBowt(rbg_index *ix) : ix_(ix, rbg_free) {
        rbg_info_t info;
        detail::check(rbg_info(ix, &info), "rbg_info");
        n_ = info.n;
        has_tsa_ = info.has_tsa;
        has_ma_ = info.has_markers;
        f_.resize(256);
        detail::check(rbg_get_f(ix, f_.data()), "rbg_get_f");
    }

    rbg_index *handle() const { return ix_.get(); }

    // rowbowt.hpp:115-118
    range_t full_range() const { return {0, n_ - 1}; }

    // rowbowt.hpp:74-88
    range_t LF(range_t rn, uint8_t c) const {
        range_t out;
        detail::check(rbg_lf(ix_.get(), &rn.first, &rn.second, &c, 1, &out.first, &out.second), "rbg_lf");
        return out;
    }
    range_t LF(uint64_t s, uint64_t e, uint8_t c) const { return LF(range_t(s, e), c); }

    // rowbowt.hpp:121-131
    range_t find_range(const std::string &query) const {
        const uint64_t off[2] = {0, query.size()};
        range_t r;
        detail::check(rbg_find_range(ix_.get(), reinterpret_cast<const uint8_t *>(query.data()), off, 1, &r.first, &r.second),
                      "rbg_find_range");
        return r;
    }

    // rowbowt.hpp:266-269
    uint64_t count(const std::string &query) const {
        auto rn = find_range(query);
        return rn.second >= rn.first ? (rn.second - rn.first) + 1 : 0;
    }

    // rowbowt.hpp:169-184
    LFData find_range_w_toehold(const std::string &query) const {
        LFData lf;
        if (!has_tsa_) return lf;  // :171
        const uint64_t off[2] = {0, query.size()};
        detail::check(rbg_find_range_w_toehold(ix_.get(), reinterpret_cast<const uint8_t *>(query.data()), off, 1,
                                               &lf.rn.first, &lf.rn.second, &lf.ssamp), "rbg_find_range_w_toehold");
        return lf;
    }

    // rowbowt.hpp:613-621 (appends to locs, like ToeholdSA::locate_range toehold_sa.hpp:37-49)
    std::vector<uint64_t> &locs_at(range_t range, uint64_t k, uint64_t max_hits, std::vector<uint64_t> &locs) const {
        uint64_t off[2];
        detail::LibBuf buf;
        detail::check(rbg_locs_at(ix_.get(), &range.first, &range.second, &k, 1, max_hits, off, &buf.p), "rbg_locs_at");
        locs.insert(locs.end(), buf.p, buf.p + off[1]);
        return locs;
    }
    std::vector<uint64_t> locs_at(range_t range, uint64_t k, uint64_t max_hits) const {
        std::vector<uint64_t> locs;
        locs_at(range, k, max_hits, locs);
        return locs;
    }

    // rowbowt.hpp:623-625
    std::pair<std::string, uint64_t> resolve_offset(uint64_t i) const {
        const char *name = nullptr;
        uint64_t off = 0;
        detail::check(rbg_resolve_offset(ix_.get(), i, &name, &off), "rbg_resolve_offset");
        return std::make_pair(std::string(name), off);
    }

    // SAM lines of a batch of raw reads (rbg_align_sam: both strands searched, the longer greedy seed located, soft-clipped records written on the device)
    // as one string; quals: a quality string per read of the read's length, or empty for QUAL "*"; names: one per read
    std::string align_sam(const std::vector<std::string> &seqs, const std::vector<std::string> &quals, const std::vector<std::string> &names,
                          uint64_t min_length = 20, uint64_t max_hits = 16, bool secondary = false) const {
        return sam_lines(seqs, quals, names, min_length, max_hits, secondary, -1);
    }
    // the same lines with every seed extended leftwards through up to max_mismatch mismatches by an LF walk (rbg_align_sam_extend: POS and the left clip move,
    // NM / MD / AS follow HI on every mapped line; there is no right extension)
    std::string align_sam_extend(const std::vector<std::string> &seqs, const std::vector<std::string> &quals, const std::vector<std::string> &names,
                                 uint64_t min_length = 20, uint64_t max_hits = 16, bool secondary = false, uint32_t max_mismatch = 4) const {
        return sam_lines(seqs, quals, names, min_length, max_hits, secondary, static_cast<int>(max_mismatch > 0x7FFFFFFFu ? 0x7FFFFFFFu : max_mismatch));
    }
    // the FL index on this handle's device (rbg_fl_prepare: idempotent, opt-in), which align_sam_extend_both needs
    void fl_prepare() { detail::check(rbg_fl_prepare(ix_.get()), "rbg_fl_prepare"); }
    // the ISA sample on this handle's device (rbg_extract_prepare: runs fl_prepare if needed; idempotent, opt-in), which isa and extract need
    void extract_prepare() { detail::check(rbg_extract_prepare(ix_.get()), "rbg_extract_prepare"); }
    // the rows of the suffixes at text positions (rbg_isa)
    std::vector<uint64_t> isa(const std::vector<uint64_t> &positions) const {
        std::vector<uint64_t> rows(positions.size());
        detail::check(rbg_isa(ix_.get(), positions.data(), positions.size(), rows.data()), "rbg_isa");
        return rows;
    }
    uint64_t isa(uint64_t position) const { return isa(std::vector<uint64_t>{position})[0]; }
    // the text of intervals (rbg_extract): text[j] holds the got[j] bases from pos[j] on -- up to len[j], ending before the first byte that is no base
    struct Extracted { std::vector<std::string> text; std::vector<uint64_t> got; };
    Extracted extract(const std::vector<uint64_t> &pos, const std::vector<uint64_t> &len) const {
        if (pos.size() != len.size()) detail::die("extract: a length per position", RBG_EARG);
        uint64_t total = 0;
        for (const uint64_t l : len) total += l;
        std::string out(total, '\0');
        Extracted r;
        r.got.resize(pos.size());
        detail::check(rbg_extract(ix_.get(), pos.data(), len.data(), pos.size(), reinterpret_cast<uint8_t *>(&out[0]), r.got.data()), "rbg_extract");
        uint64_t at = 0;
        for (size_t j = 0; j < pos.size(); at += len[j], ++j) r.text.push_back(out.substr(at, r.got[j]));
        return r;
    }
    std::string extract(uint64_t pos, uint64_t len) const { return extract(std::vector<uint64_t>{pos}, std::vector<uint64_t>{len}).text[0]; }
    // align_sam_extend's lines with the right clip extended too, by an FL walk with what the left walk left of the budget (rbg_align_sam_extend_both)
    std::string align_sam_extend_both(const std::vector<std::string> &seqs, const std::vector<std::string> &quals, const std::vector<std::string> &names,
                                      uint64_t min_length = 20, uint64_t max_hits = 16, bool secondary = false, uint32_t max_mismatch = 4) const {
        return sam_lines(seqs, quals, names, min_length, max_hits, secondary, static_cast<int>(max_mismatch > 0x7FFFFFFFu ? 0x7FFFFFFFu : max_mismatch), true);
    }

  private:
    std::string sam_lines(const std::vector<std::string> &seqs, const std::vector<std::string> &quals, const std::vector<std::string> &names, uint64_t min_length,
                          uint64_t max_hits, bool secondary, int max_mismatch /* < 0: rbg_align_sam */, bool right = false) const {
        const uint64_t N = seqs.size();
        if (names.size() != N || (!quals.empty() && quals.size() != N)) detail::die("align_sam: a name (and a quality string, if any) per read", RBG_EARG);
        std::string sblob, qblob, nblob;
        std::vector<uint64_t> sbeg(N), nbeg(N);
        std::vector<uint32_t> slen(N), nlen(N);
        for (uint64_t i = 0; i < N; ++i) {
            if (!quals.empty() && quals[i].size() != seqs[i].size()) detail::die("align_sam: a quality string of the read's length", RBG_EARG);
            sbeg[i] = sblob.size(); slen[i] = static_cast<uint32_t>(seqs[i].size()); sblob += seqs[i];
            if (!quals.empty()) qblob += quals[i];
            nbeg[i] = nblob.size(); nlen[i] = static_cast<uint32_t>(names[i].size()); nblob += names[i];
        }
        const char *text = nullptr;
        uint64_t n = 0;
        if (max_mismatch < 0)
            detail::check(rbg_align_sam(ix_.get(), sblob.data(), sbeg.data(), slen.data(), quals.empty() ? nullptr : qblob.data(), sbeg.data(), nblob.data(),
                                        nbeg.data(), nlen.data(), N, min_length, max_hits, secondary ? RBG_SAM_SECONDARY : 0u, &text, &n), "rbg_align_sam");
        else if (right)
            detail::check(rbg_align_sam_extend_both(ix_.get(), sblob.data(), sbeg.data(), slen.data(), quals.empty() ? nullptr : qblob.data(), sbeg.data(),
                                                    nblob.data(), nbeg.data(), nlen.data(), N, min_length, max_hits, secondary ? RBG_SAM_SECONDARY : 0u,
                                                    static_cast<uint32_t>(max_mismatch), &text, &n), "rbg_align_sam_extend_both");
        else
            detail::check(rbg_align_sam_extend(ix_.get(), sblob.data(), sbeg.data(), slen.data(), quals.empty() ? nullptr : qblob.data(), sbeg.data(), nblob.data(),
                                               nbeg.data(), nlen.data(), N, min_length, max_hits, secondary ? RBG_SAM_SECONDARY : 0u,
                                               static_cast<uint32_t>(max_mismatch), &text, &n), "rbg_align_sam_extend");
        const int rc = rbg_wait_text(ix_.get(), text);
        std::string out = rc == RBG_OK && n ? std::string(text, n) : std::string();
        (void)rbg_release_text(ix_.get(), text);
        detail::check(rc, "rbg_wait_text");
        return out;
    }

  public:
    std::string align_sam(const std::vector<std::string> &seqs, const std::vector<std::string> &names) const { return align_sam(seqs, {}, names); }
    // the header that goes with those lines (rbg_sam_header): @HD, one @SQ per document, then pg_line as given
    std::string sam_header(const std::string &pg_line = std::string()) const {
        char *text = nullptr;
        uint64_t n = 0;
        detail::check(rbg_sam_header(ix_.get(), pg_line.empty() ? nullptr : pg_line.c_str(), &text, &n), "rbg_sam_header");
        std::string out(text, n);
        rbg_free_buffer(text);
        return out;
    }

    // resolve_offset for many positions that are in HOST memory: one fetch of the table (rbg_doc_table) and the rule of doclist.hpp:46-50, :77-79 (rbg_docdir.hpp) per position,
    // instead of a call through the ABI each.  doc[i] = the document's index into names() of rbg_doc_table, RBG_DOC_NONE where position i has none (the single
    // call exits there; the offset is then the position itself).  Positions that are on the device go through rbg_resolve_offsets_dev and never come here.
    struct DocOffsets { std::vector<uint32_t> doc; std::vector<uint64_t> offset; std::vector<std::string> names; };
    DocOffsets resolve_offsets(const std::vector<uint64_t> &positions) const {
        uint64_t nd = 0, size = 0;
        const uint64_t *sorted = nullptr;
        const char *const *names = nullptr;
        detail::check(rbg_doc_table(ix_.get(), &nd, &sorted, &names, &size), "rbg_doc_table");
        DocOffsets r;
        r.names.assign(names, names + nd);
        r.doc.resize(positions.size());
        r.offset.resize(positions.size());
        for (size_t i = 0; i < positions.size(); ++i) {
            const uint64_t l = positions[i], j = rbg::doc_rank_search(sorted, nd, size, l);
            r.doc[i] = j ? static_cast<uint32_t>(j - 1) : RBG_DOC_NONE;
            r.offset[i] = j ? l - sorted[j - 1] : l;
        }
        return r;
    }
    // Which documents each read's locations fall in (rbg_doc_hits): find_range_w_toehold + locs_at(max_hits) + resolve_offset reduced per read on the device,
    // the locations never crossing to the host.  sets[i * words + d / 64] bit d % 64 = read i has a location in document d; doc_reads[d] = reads of this batch
    // with a location in document d (a read counts once per document).
    struct DocHits {
        std::vector<range_t> ranges;
        uint64_t words = 0;                 // u64 words per read in `sets`: ceil(documents / 64)
        std::vector<uint64_t> sets;         // [reads * words]
        std::vector<uint32_t> ndocs, nodoc; // distinct documents per read; its locations that have no document
        std::vector<uint64_t> doc_reads;    // [documents]
        bool hit(uint64_t read, uint64_t d) const { return (sets[read * words + d / 64] >> (d % 64)) & 1u; }
    };
    // the same with the LOCATIONS per document (rbg_doc_hits_locs): doc_locs[d] = the locations of this batch that fall in document d; their sum plus the sum
    // of nodoc is the number of locations locs_at(max_hits) would have returned
    DocHits doc_hits(const std::vector<std::string> &queries, uint64_t max_hits, std::vector<uint64_t> &doc_locs) const {
        return doc_hits_impl(queries, max_hits, &doc_locs);
    }
    DocHits doc_hits(const std::vector<std::string> &queries, std::vector<uint64_t> &doc_locs) const {
        return doc_hits_impl(queries, static_cast<uint64_t>(-1), &doc_locs);
    }
    DocHits doc_hits(const std::vector<std::string> &queries, uint64_t max_hits = static_cast<uint64_t>(-1)) const {
        return doc_hits_impl(queries, max_hits, nullptr);
    }
    DocHits doc_hits_impl(const std::vector<std::string> &queries, uint64_t max_hits, std::vector<uint64_t> *doc_locs) const {
        detail::Batch b;
        for (const auto &q : queries) b.add(q);
        const uint64_t N = b.size();
        detail::check(rbg_docs_prepare(ix_.get()), "rbg_docs_prepare");
        uint64_t nd = 0, size = 0;
        const uint64_t *sorted = nullptr;
        const char *const *names = nullptr;
        detail::check(rbg_doc_table(ix_.get(), &nd, &sorted, &names, &size), "rbg_doc_table");
        DocHits r;
        r.words = rbg_doc_hits_words(ix_.get());
        std::vector<uint64_t> lo(N), hi(N);
        r.sets.assign(N * r.words, 0);
        r.ndocs.assign(N, 0);
        r.nodoc.assign(N, 0);
        r.doc_reads.assign(nd, 0);
        if (doc_locs) {
            doc_locs->assign(nd, 0);
            detail::check(rbg_doc_hits_locs(ix_.get(), b.data(), b.off.data(), N, max_hits, lo.data(), hi.data(), r.sets.data(), r.ndocs.data(), r.nodoc.data(),
                                            r.doc_reads.data(), doc_locs->data()), "rbg_doc_hits_locs");
        } else {
            detail::check(rbg_doc_hits(ix_.get(), b.data(), b.off.data(), N, max_hits, lo.data(), hi.data(), r.sets.data(), r.ndocs.data(), r.nodoc.data(),
                                       r.doc_reads.data()), "rbg_doc_hits");
        }
        r.ranges.resize(N);
        for (uint64_t i = 0; i < N; ++i) r.ranges[i] = {lo[i], hi[i]};
        return r;
    }

    // rowbowt.hpp:272-290 ("WARNING: does not clear markers!")
    std::vector<MarkerT> &markers_at(range_t r, std::vector<MarkerT> &markers) const {
        if (!has_ma_) return markers;  // :283
        uint64_t off[2];
        detail::LibBuf buf;
        detail::check(rbg_markers_at(ix_.get(), &r.first, &r.second, 1, off, &buf.p), "rbg_markers_at");
        markers.insert(markers.end(), buf.p, buf.p + off[1]);
        return markers;
    }
    std::vector<MarkerT> markers_at(range_t r) const {
        std::vector<MarkerT> markers;
        return markers_at(r, markers);
    }
    std::vector<MarkerT> &markers_at(uint64_t i, std::vector<MarkerT> &markers) const { return markers_at(range_t(i, i), markers); }
    std::vector<MarkerT> markers_at(uint64_t i) const { return markers_at(range_t(i, i)); }

    // rowbowt.hpp:292-339
    LFData find_range_w_markers(const std::string query, uint64_t wsize, uint64_t max_range) const {
        LFData lf;
        if (!has_ma_) {
            std::cerr << "warning: no marker array found!\n";  // :295
            return lf;
        }
        if (query.size() < wsize) {
            std::cerr << "warning: query (size=" << query.size() << ") is less than wsize (" << wsize << ")\n";  // :300
            return lf;
        }
        const uint64_t off[2] = {0, query.size()};
        uint64_t mk_off[2];
        detail::LibBuf buf;
        detail::check(rbg_find_range_w_markers(ix_.get(), reinterpret_cast<const uint8_t *>(query.data()), off, 1, wsize,
                                               max_range, &lf.rn.first, &lf.rn.second, mk_off, &buf.p),
                      "rbg_find_range_w_markers");
        lf.markers.assign(buf.p, buf.p + mk_off[1]);
        if (lf.rn.second >= lf.rn.first) { lf.qstart = 0; lf.qend = query.size(); }  // :336-337
        return lf;
    }

    // rowbowt.hpp:406-482: fn(range, (q.first, q.second), mbuf) once per seed, right to left, exactly as the
    // reference calls it (q.second = q.first - 1, wrapped, for an empty seed); goes through the ftab when
    // one was loaded with LoadRbwtFlag::FT and not disabled (:430)
    template <typename F>
    void get_markers_greedy_seeding(const std::string query, uint64_t wsize, uint64_t max_range, F fn) const {
        const uint64_t ft_k = disable_ft_ ? 0 : ft_k_;
        if (ft_k_ && ft_k_ - 1 > wsize) {  // :423-426
            std::cerr << "ERROR: wsize cannot be greater than or equal to ftab k size. please rebuild ftab with smaller k\n";
            std::exit(1);
        }
        if (ft_k && query.size() < ft_k) {  // std::string::substr(pos > size()) throws in the reference (:431)
            std::cerr << "rowbowt_gpu: query shorter than the ftab k-mer size" << std::endl;
            std::exit(1);
        }
        const uint64_t off[2] = {0, query.size()};
        uint64_t seed_off[2];
        rbg_marker_seed_t *seeds = nullptr;
        detail::LibBuf mk;
        detail::check(rbg_get_markers_greedy_seeding(ix_.get(), reinterpret_cast<const uint8_t *>(query.data()), off, 1, wsize,
                                                     max_range, ft_k, seed_off, &seeds, &mk.p), "rbg_get_markers_greedy_seeding");
        std::unique_ptr<rbg_marker_seed_t, void (*)(void *)> hold(seeds, rbg_free_buffer);
        for (uint64_t s = 0; s < seed_off[1]; ++s) {
            const rbg_marker_seed_t &d = seeds[s];
            fn(range_t(d.lo, d.hi), std::make_pair(static_cast<size_t>(d.qstart), static_cast<size_t>(d.qend - 1)),
               std::vector<MarkerT>(mk.p + d.mk_begin, mk.p + d.mk_end));
        }
    }

    // rowbowt.hpp:341-404: fn(range, (q.first, q.second), mbuf) for every end position m, m-1, ..., 1 of the query, exactly as
    // the reference calls it.  A failed extension is reported twice there: fn(prev_range, q, mbuf) (:389), then, after the
    // break, fn(range, q, mbuf) (:402) with LF's empty range and the cleared mbuf.  The second call is replayed here with the
    // library's in-band empty range {1, 0} (LF's own empty pair depends on the ranks where the search died).  The per-step
    // debug text the reference prints to stderr is not reproduced.
    template <typename F>
    void get_markers_lmems(const std::string query, uint64_t wsize, uint64_t max_range, F fn) const {
        if (disable_ft_ || !ft_k_) {  // :346-349
            std::cerr << "ftab must be enabled!" << std::endl;
            std::exit(1);
        }
        if (ft_k_ - 1 > wsize) {  // :350-353
            std::cerr << "ERROR: wsize cannot be greater than or equal to ftab k size. please rebuild ftab with smaller k\n";
            std::exit(1);
        }
        const uint64_t off[2] = {0, query.size()};
        uint64_t seed_off[2];
        rbg_marker_seed_t *seeds = nullptr;
        detail::LibBuf mk;
        detail::check(rbg_get_markers_lmems(ix_.get(), reinterpret_cast<const uint8_t *>(query.data()), off, 1, wsize, max_range, ft_k_,
                                            seed_off, &seeds, &mk.p), "rbg_get_markers_lmems");
        std::unique_ptr<rbg_marker_seed_t, void (*)(void *)> hold(seeds, rbg_free_buffer);
        for (uint64_t s = 0; s < seed_off[1]; ++s) {
            const rbg_marker_seed_t &d = seeds[s];
            const auto q = std::make_pair(static_cast<size_t>(d.qstart), static_cast<size_t>(d.qend - 1));
            fn(range_t(d.lo, d.hi), q, std::vector<MarkerT>(mk.p + d.mk_begin, mk.p + d.mk_end));
            if (d.qstart > 0) fn(range_t(1, 0), q, std::vector<MarkerT>());   // the failed extension's second call (:402)
        }
    }

    // rowbowt.hpp:633-662 (get_seeds_greedy_w_sample :222-256 + locate_from_longest_seed :664-685)
    std::vector<uint64_t> &find_locs_greedy_seeding(std::string s, uint64_t min_length, uint64_t max_hits,
                                                    std::vector<uint64_t> &locs) const {
        locs.clear();
        if (!has_tsa_) return locs;
        const uint64_t off[2] = {0, s.size()};
        uint64_t loc_off[2];
        detail::LibBuf buf;
        detail::check(rbg_find_locs_greedy_seeding(ix_.get(), reinterpret_cast<const uint8_t *>(s.data()), off, 1, min_length,
                                                   max_hits, loc_off, &buf.p), "rbg_find_locs_greedy_seeding");
        locs.assign(buf.p, buf.p + loc_off[1]);
        return locs;
    }
    std::vector<uint64_t> find_locs_greedy_seeding(std::string s, uint64_t min_length, uint64_t max_hits) const {
        std::vector<uint64_t> locs;
        return find_locs_greedy_seeding(s, min_length, max_hits, locs);
    }
    // rowbowt.hpp:191-215: every greedy seed of the query, the rightmost first; the last record (qstart 0) is always pushed.
    // ssamp is 0 (the reference leaves it unset); works without a toehold SA
    std::vector<LFData> &get_seeds_greedy(const std::string &query, uint64_t min_length, std::vector<LFData> &lfdata) const {
        return seed_list(query, min_length, 0u, lfdata);
    }
    // rowbowt.hpp:222-256: the same with the toehold of every seed; the last record only if it has min_length symbols;
    // no toehold SA: an empty list (:225)
    std::vector<LFData> &get_seeds_greedy_w_sample(const std::string &query, uint64_t min_length, std::vector<LFData> &lfdata) const {
        lfdata.clear();
        if (!has_tsa_) return lfdata;
        return seed_list(query, min_length, RBG_SEEDS_W_SAMPLE, lfdata);
    }
    std::vector<LFData> get_seeds_greedy_w_sample(const std::string &query, uint64_t min_length) const {
        std::vector<LFData> lfs;
        return get_seeds_greedy_w_sample(query, min_length, lfs);
    }

    // rowbowt.hpp:575-611: a record after step wsize, 2 wsize, ... of the backward search (labelled one symbol behind its range
    // and toehold, include/rbg.h) and the whole query's at the end when (m - 1) % wsize != 0; empty when the query does not
    // occur or there is no toehold SA.  wsize == 0 (the reference divides by it) ends the program with the library's error
    std::vector<LFData> &find_range_w_toehold_chkpnts(const std::string &query, uint64_t wsize, std::vector<LFData> &lfs) const {
        lfs.clear();
        if (!has_tsa_) return lfs;  // :579
        const uint64_t off[2] = {0, query.size()};
        uint64_t seed_off[2];
        detail::LibBuf buf;
        detail::check(rbg_find_range_w_toehold_chkpnts(ix_.get(), reinterpret_cast<const uint8_t *>(query.data()), off, 1, wsize, seed_off,
                                                       &buf.p), "rbg_find_range_w_toehold_chkpnts");
        append_records(buf.p, seed_off[1], 0, seed_off[1], lfs);
        return lfs;
    }
    std::vector<LFData> find_range_w_toehold_chkpnts(const std::string &query, uint64_t wsize) const {
        std::vector<LFData> lfs;
        return find_range_w_toehold_chkpnts(query, wsize, lfs);
    }

    // rowbowt.hpp:664-690: the first seed of strictly greatest length, then locs_at, then minus its qstart; an empty list, or
    // zero-length seeds only (best_range stays the default LFData, an empty range), gives no locations
    std::vector<uint64_t> &locate_from_longest_seed(uint64_t max_hits, const std::vector<LFData> &lfs, std::vector<uint64_t> &locs) const {
        locs.clear();
        const LFData *best = nullptr;
        uint64_t max_length = 0;
        for (const auto &lfd : lfs) {
            const uint64_t length = lfd.qend - lfd.qstart;
            if (length > max_length) { max_length = length; best = &lfd; }
        }
        if (!best) return locs;
        locs_at(best->rn, best->ssamp, max_hits, locs);
        for (auto &l : locs) l -= best->qstart;
        return locs;
    }
    std::vector<uint64_t> locate_from_longest_seed(uint64_t max_hits, const std::vector<LFData> &lfs) {
        std::vector<uint64_t> locs;
        return locate_from_longest_seed(max_hits, lfs, locs);
    }

    // the seed locate_from_longest_seed would pick among get_seeds_greedy_w_sample(query, min_length)
    LFData longest_greedy_seed(const std::string &query, uint64_t min_length) const {
        LFData lf;
        if (!has_tsa_) return lf;
        const uint64_t off[2] = {0, query.size()};
        detail::check(rbg_greedy_longest_seed(ix_.get(), reinterpret_cast<const uint8_t *>(query.data()), off, 1, min_length,
                                              &lf.rn.first, &lf.rn.second, &lf.qstart, &lf.qend, &lf.ssamp), "rbg_greedy_longest_seed");
        return lf;
    }

    const std::vector<uint64_t> &get_f() const { return f_; }  // rowbowt.hpp:719

    // ftab (LoadRbwtFlag::FT): find_range is result-neutral under it (rowbowt.hpp:124-125); the marker-seed
    // variant is not.  load_ftab verifies the file is build_ftab(k) of this index and keeps k (ftab.hpp:15-27).
    void load_ftab(const std::string &fname) {
        const int rc = rbg_check_ftab(ix_.get(), fname.c_str(), &ft_k_);
        if (rc == RBG_EIO) { std::cerr << "bad file" << std::endl; std::exit(1); }  // rowbowt_io.hpp:167
        detail::check(rc, "load_ftab (the .ftab must be the one rb_build -f made for this index)");
    }
    uint64_t ftab_k() const { return ft_k_; }
    // the marker index keyed by text position, <prefix>.midx (rle_window_arr::load, rb_markers_tsa.cpp:99-101): what
    // find_loc_markers_greedy_seeding_batch answers from.  A missing file exits 1 with a message.
    void load_text_markers(const std::string &fname) {
        const int rc = rbg_load_text_markers(ix_.get(), fname.c_str());
        if (rc == RBG_EIO) { std::cerr << "bad file: " << fname << std::endl; std::exit(1); }
        detail::check(rc, "load_text_markers");
    }
    void disable_ft() { disable_ft_ = true; }   // rowbowt.hpp:760-766
    void enable_ft() { disable_ft_ = false; }

    // ---- batched forms (one launch for all reads) ------------------------------------------------
    void find_range_batch(const std::vector<std::string> &queries, std::vector<range_t> &out) const {
        detail::Batch b;
        for (const auto &q : queries) b.add(q);
        std::vector<uint64_t> lo(b.size()), hi(b.size());
        detail::check(rbg_find_range(ix_.get(), b.data(), b.off.data(), b.size(), lo.data(), hi.data()), "rbg_find_range");
        out.resize(b.size());
        for (uint64_t i = 0; i < b.size(); ++i) out[i] = {lo[i], hi[i]};
    }
    void find_range_w_toehold_batch(const std::vector<std::string> &queries, std::vector<LFData> &out) const {
        out.assign(queries.size(), LFData());
        if (!has_tsa_) return;
        detail::Batch b;
        for (const auto &q : queries) b.add(q);
        std::vector<uint64_t> lo(b.size()), hi(b.size()), k(b.size());
        detail::check(rbg_find_range_w_toehold(ix_.get(), b.data(), b.off.data(), b.size(), lo.data(), hi.data(), k.data()),
                      "rbg_find_range_w_toehold");
        for (uint64_t i = 0; i < b.size(); ++i) { out[i].rn = {lo[i], hi[i]}; out[i].ssamp = k[i]; }
    }
    // locs_at for many (range, toehold) triples: loc_off[N+1] + concatenated locations
    void locs_at_batch(const std::vector<LFData> &lfs, uint64_t max_hits, std::vector<uint64_t> &loc_off,
                       std::vector<uint64_t> &locs) const {
        const uint64_t N = lfs.size();
        std::vector<uint64_t> lo(N), hi(N), k(N);
        for (uint64_t i = 0; i < N; ++i) { lo[i] = lfs[i].rn.first; hi[i] = lfs[i].rn.second; k[i] = lfs[i].ssamp; }
        loc_off.assign(N + 1, 0);
        detail::LibBuf buf;
        detail::check(rbg_locs_at(ix_.get(), lo.data(), hi.data(), k.data(), N, max_hits, loc_off.data(), &buf.p), "rbg_locs_at");
        locs.assign(buf.p, buf.p + loc_off[N]);
    }
    void markers_at_batch(const std::vector<range_t> &ranges, std::vector<uint64_t> &mk_off, std::vector<MarkerT> &mk) const {
        const uint64_t N = ranges.size();
        mk_off.assign(N + 1, 0);
        mk.clear();
        if (!has_ma_) return;
        std::vector<uint64_t> lo(N), hi(N);
        for (uint64_t i = 0; i < N; ++i) { lo[i] = ranges[i].first; hi[i] = ranges[i].second; }
        detail::LibBuf buf;
        detail::check(rbg_markers_at(ix_.get(), lo.data(), hi.data(), N, mk_off.data(), &buf.p), "rbg_markers_at");
        mk.assign(buf.p, buf.p + mk_off[N]);
    }

    // rb_markers_tsa.cpp:76-88 for many reads: find_locs_greedy_seeding(query, min_length, max_hits), and for every location l the markers
    // midx.at_range(l, l + query.size() - 1); locs / mk are concatenated per read (loc_off / mk_off, N + 1 each), a read's markers in the
    // order of its locations.  Needs load_text_markers; without a toehold SA every list is empty, as find_locs_greedy_seeding's are.
    void find_loc_markers_greedy_seeding_batch(const std::vector<std::string> &queries, uint64_t min_length, uint64_t max_hits,
                                               std::vector<uint64_t> &loc_off, std::vector<uint64_t> &locs, std::vector<uint64_t> &mk_off,
                                               std::vector<MarkerT> &mk) const {
        const uint64_t N = queries.size();
        loc_off.assign(N + 1, 0);
        mk_off.assign(N + 1, 0);
        locs.clear();
        mk.clear();
        if (!has_tsa_) return;
        detail::Batch b;
        for (const auto &q : queries) b.add(q);
        detail::LibBuf lbuf, mbuf;
        detail::check(rbg_find_loc_markers_greedy_seeding(ix_.get(), b.data(), b.off.data(), N, min_length, max_hits, loc_off.data(), &lbuf.p,
                                                          mk_off.data(), &mbuf.p), "rbg_find_loc_markers_greedy_seeding");
        locs.assign(lbuf.p, lbuf.p + loc_off[N]);
        mk.assign(mbuf.p, mbuf.p + mk_off[N]);
    }

    // What rb_markers prints for many RAW reads (rb_markers.cpp:357-519: both strands, the seeding, out_fn's sort + unique, the heuristic
    // worker's filters and choices), as records: read i prints seeds[seed_off[i] .. seed_off[i + 1]) in that order, a record's markers are
    // mk[mk_begin .. mk_end), sorted by marker_cmp and unique.  params.ftab_k is set to the loaded ftab's k; first_fwd: the heuristic worker's
    // coin per read (empty: forward first).  Exits like the reference where it would (ftab k - 1 > wsize, lmem without an ftab).
    void markers_report_batch(const std::vector<std::string> &queries, rbg_report_params_t params, const std::vector<uint8_t> &first_fwd,
                              std::vector<uint64_t> &seed_off, std::vector<rbg_report_seed_t> &seeds, std::vector<MarkerT> &mk) const {
        const uint64_t N = queries.size();
        params.ftab_k = disable_ft_ ? 0 : ft_k_;
        seed_off.assign(N + 1, 0);
        detail::Batch b;
        for (const auto &q : queries) b.add(q);
        rbg_report_seed_t *recs = nullptr;
        detail::LibBuf mbuf;
        detail::check(rbg_markers_report(ix_.get(), b.data(), b.off.data(), N, first_fwd.size() == N && N ? first_fwd.data() : nullptr, &params,
                                         seed_off.data(), &recs, &mbuf.p), "rbg_markers_report");
        std::unique_ptr<rbg_report_seed_t, void (*)(void *)> hold(recs, rbg_free_buffer);
        seeds.assign(recs, recs + seed_off[N]);
        mk.assign(mbuf.p, mbuf.p + (seed_off[N] ? recs[seed_off[N] - 1].mk_end : 0));
    }

    // The same reads and parameters as markers_report_batch, but the printed lines' markers are counted on the device into `tally` (made by
    // make_tally of this index) instead of coming back: n_fwd / n_rev per strand of the line, len_sum of the lines' query_len.  tally_flags:
    // RBG_TALLY_PER_READ counts a marker once per read (its longest line), | RBG_TALLY_DROP_SITE_CONFLICTS leaves out the sites of which a read
    // carries two alleles (include/rbg.h).
    MarkerTally make_tally(uint64_t distinct_hint = 0) const { return MarkerTally(ix_.get(), distinct_hint); }
    void markers_tally(const std::vector<std::string> &queries, rbg_report_params_t params, const std::vector<uint8_t> &first_fwd, MarkerTally &tally,
                       uint32_t tally_flags = 0) const {
        const uint64_t N = queries.size();
        params.ftab_k = disable_ft_ ? 0 : ft_k_;
        detail::Batch b;
        for (const auto &q : queries) b.add(q);
        detail::check(rbg_markers_tally_reads(ix_.get(), b.data(), b.off.data(), N, first_fwd.size() == N && N ? first_fwd.data() : nullptr, &params, tally_flags,
                                              tally.handle()),
                      "rbg_markers_tally_reads");
    }

    // get_seeds_greedy_w_sample (w_sample) or get_seeds_greedy for many reads: out[i] = the list of queries[i]
    void get_seeds_greedy_batch(const std::vector<std::string> &queries, uint64_t min_length, bool w_sample,
                                std::vector<std::vector<LFData>> &out) const {
        out.assign(queries.size(), std::vector<LFData>());
        if (w_sample && !has_tsa_) return;
        detail::Batch b;
        for (const auto &q : queries) b.add(q);
        std::vector<uint64_t> seed_off(b.size() + 1);
        detail::LibBuf buf;
        detail::check(rbg_get_seeds_greedy(ix_.get(), b.data(), b.off.data(), b.size(), min_length, w_sample ? RBG_SEEDS_W_SAMPLE : 0u,
                                           seed_off.data(), &buf.p), "rbg_get_seeds_greedy");
        for (uint64_t i = 0; i < b.size(); ++i) append_records(buf.p, seed_off[b.size()], seed_off[i], seed_off[i + 1], out[i]);
    }
    void find_range_w_toehold_chkpnts_batch(const std::vector<std::string> &queries, uint64_t wsize, std::vector<std::vector<LFData>> &out) const {
        out.assign(queries.size(), std::vector<LFData>());
        if (!has_tsa_) return;
        detail::Batch b;
        for (const auto &q : queries) b.add(q);
        std::vector<uint64_t> seed_off(b.size() + 1);
        detail::LibBuf buf;
        detail::check(rbg_find_range_w_toehold_chkpnts(ix_.get(), b.data(), b.off.data(), b.size(), wsize, seed_off.data(), &buf.p),
                      "rbg_find_range_w_toehold_chkpnts");
        for (uint64_t i = 0; i < b.size(); ++i) append_records(buf.p, seed_off[b.size()], seed_off[i], seed_off[i + 1], out[i]);
    }

   private:
    // records [from, to) of a library block of five arrays of `total` entries (lo | hi | qstart | qend | ssamp)
    static void append_records(const uint64_t *p, uint64_t total, uint64_t from, uint64_t to, std::vector<LFData> &lfs) {
        for (uint64_t t = from; t < to; ++t)
            lfs.push_back(LFData(range_t(p[t], p[total + t]), p[2 * total + t], p[3 * total + t], p[4 * total + t]));
    }
    std::vector<LFData> &seed_list(const std::string &query, uint64_t min_length, uint32_t flags, std::vector<LFData> &lfdata) const {
        lfdata.clear();
        const uint64_t off[2] = {0, query.size()};
        uint64_t seed_off[2];
        detail::LibBuf buf;
        detail::check(rbg_get_seeds_greedy(ix_.get(), reinterpret_cast<const uint8_t *>(query.data()), off, 1, min_length, flags, seed_off,
                                           &buf.p), "rbg_get_seeds_greedy");
        append_records(buf.p, seed_off[1], 0, seed_off[1], lfdata);
        return lfdata;
    }

    std::shared_ptr<rbg_index> ix_;
    uint64_t n_ = 0;
    bool has_tsa_ = false, has_ma_ = false, disable_ft_ = false;
    uint64_t ft_k_ = 0;
    std::vector<uint64_t> f_;
};

// rowbowt_io.hpp:176-189.  `device` is the only addition (defaults to HIP device 0).
template <typename StringT = rle_string_t>
RowBowt<StringT> load_rowbowt(std::string prefix, LoadRbwtFlag flag, int device = 0) {
    std::cerr << "loading type: rbg flat index (MI355X)" << std::endl;  // cf. rowbowt_io.hpp:180
    rbg_index *ix = nullptr;
    const int rc = rbg_load(prefix.c_str(), static_cast<int>(flag), device, &ix);
    if (rc == RBG_EIO) {
        std::cerr << "bad file" << std::endl;  // rowbowt_io.hpp:167
        std::exit(1);
    }
    detail::check(rc, "load_rowbowt");
    RowBowt<StringT> rb(ix);
    if (static_cast<int>(flag & LoadRbwtFlag::FT)) rb.load_ftab(prefix + ".ftab");  // rowbowt_io.hpp:21,187
    return rb;
}

// The index of a text in memory (rbg_build_from_text): `text` ends in its unique smallest byte -- rb_build --fasta's text is the documents joined by '#'
// and a final 0x01 --; the suffix array, the BWT's runs and their samples are made on the device.  The reference has no builder from a text (its rb_build
// starts from pfbwt-f's files, rb_build.cpp:83-93).  LoadRbwtFlag::SA keeps the toehold samples.
template <typename StringT = rle_string_t>
RowBowt<StringT> build_from_text(const std::string &text, LoadRbwtFlag flag = LoadRbwtFlag::SA, int device = 0) {
    rbg_index *ix = nullptr;
    detail::check(rbg_build_from_text(reinterpret_cast<const uint8_t *>(text.data()), text.size(), static_cast<int>(flag), device, &ix), "build_from_text");
    return RowBowt<StringT>(ix);
}

// The same with the marker array made from site records (rbg_build_from_text_markers; include/rbg.h states the rule): pos, first and val of one length,
// windows of w bases.  No records: the build above.
template <typename StringT = rle_string_t>
RowBowt<StringT> build_from_text(const std::string &text, const std::vector<uint64_t> &pos, const std::vector<uint64_t> &first, const std::vector<uint64_t> &val,
                                 uint32_t w, LoadRbwtFlag flag = LoadRbwtFlag::SA, int device = 0) {
    if (pos.size() != first.size() || pos.size() != val.size()) detail::check(RBG_EARG, "build_from_text");
    rbg_index *ix = nullptr;
    detail::check(rbg_build_from_text_markers(reinterpret_cast<const uint8_t *>(text.data()), text.size(), pos.data(), first.data(), val.data(), pos.size(), w,
                                              static_cast<int>(flag), device, &ix),
                  "build_from_text");
    return RowBowt<StringT>(ix);
}

}  // namespace rbwt
