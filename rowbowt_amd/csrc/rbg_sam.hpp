// rbg_sam.hpp -- the rules of rbg_align_sam's SAM lines and of rbg_sam_header's text, stated once for host and device (k_sam.hip formats lines with
// sam_put_line, capi/sam.ipp builds the header with sam_header_text; a host compiler takes this file alone: tests/cpp/sam_host_check.cpp).
//
// COMPLEMENT.  ACGTacgt -> TGCAtgca, every other byte is itself.  This is not seq_ntoa_table (k_report.hip): an N stays N and ends a seed.
//
// CIGAR.  A read of m bytes whose seed is [a, b) in the searched orientation: [a "S"] (b - a) "M" [(m - b) "S"], zero-length operations left out.
//
// LINES (fields separated by tabs, "\n" at the end):
//   mapped     QNAME FLAG RNAME POS 255 CIGAR * 0 0 SEQ QUAL NH:i:<occ> HI:i:<j>     FLAG = (reverse ? 16 : 0) | (j > 1 ? 256 : 0); j > 1: SEQ and QUAL are "*"
//   unmapped   QNAME 4 * 0 0 * * 0 0 SEQ QUAL                                         the read as given; an empty read has SEQ "*" and QUAL "*"
// SEQ of a reverse-strand primary line is the complement of the read's bytes taken backwards, its QUAL the quality bytes taken backwards; QUAL is "*"
// when the call has no qualities.  POS is 1 + the offset of the seed's own text position in its document (nothing is subtracted for the clipped
// bases), and the document is that of this first aligned base: a seed that runs over a document boundary is NOT detected.
//
// LEFT EXTENSION (rbg_align_sam_extend, rbg_extend_left_dev; sam_extend.hip walks it, one lane per line).  Inputs of one line: the searched orientation s of
// the read (m bytes), the seed [a, b), the line's row r0 (line j of the range [lo, hi] is row hi - (j - 1)), offs = its location's offset in its document,
// the budget K (0 <= K <= RBG_SAM_MAX_MISMATCH).
//     L = min(a, offs)                       never leaves the read, never crosses the document's start
//     score = best = 0; e = 0; nm = 0; mm = 0; r = r0
//     for t in 0 .. L-1:
//         c = BWT[r]                         one of the bytes A C G T, else stop (terminator, separator, N, anything else)
//         x = s[a-1-t]                       bytes compared as they are: a lower-case or N read base is a mismatch
//         if c == x: score += 1
//         else: mm += 1; if mm > K: stop     the (K+1)-th mismatch is not taken
//               score -= 4; remember (t, c)
//         if score >= best: best = score; e = t + 1; nm = mm
//         r = LF(r, c)                       the one-row range [r, r] stepped by c
// e is the extension: it ends on a match, trailing mismatches fall away; nm counts the mismatches inside it; AS = (b - a) + best.  `steps` counts the bases
// taken (every iteration that reaches its LF).  The record lists EVERY taken mismatch in the order met (mm of them; the first nm lie inside the extension).
// The extended line: POS = offs + 1 - e, CIGAR [(a-e)S] (b-a+e)M [(m-b)S], and after HI:i: the tags NM:i:<nm>, MD:Z:<...> over the read positions [a-e, b)
// (match counts separated by the reference base of each mismatch; it starts and ends with a number) and AS:i:<AS> -- on every mapped line, also at e = 0.
// THERE IS NO RIGHT EXTENSION: LF only goes left and the index holds no FL structure; the right flank stays soft-clipped.
//
// RIGHT EXTENSION (rbg_align_sam_extend_both, rbg_extend_right_dev; fl_extend.hip walks it over the FL index of rbg_fl.hpp, which rbg_fl_prepare builds).  The
// same rule with two substitutions: x = s[b + t] for t in 0 .. L-1, L = min(m - b, limit); the reference base is the F symbol of the current row and the
// row moves by FL.  The walk starts at the line's own row (the occurrence of the seed's first base) and first takes skip = b - a FL steps without
// comparing, which crosses the seed; a row without a base on the way ends the item with a zero extension.  limit = doc_end - (location + (b - a)), doc_end the
// next sorted document start (n for the last document); the budget is K - nm of the line's left walk, so NM never exceeds K and the left walk is the one
// above, unchanged.  Lines without a right clip (m == b) make no walk.  The line: POS as the left rule gives it, CIGAR [(a-eL)S] (b-a+eL+eR)M [(m-b-eR)S],
// NM = nmL + nmR, MD over [a-eL, b+eR) (left part, seed, right part), AS = (b-a) + bestL + bestR.  The strand pick (the longer SEED) is unchanged, and a seed
// that spans a document boundary stays undetected.
//
// HEADER.  "@HD\tVN:1.6\tSO:unsorted\n", then per document in sorted-start order "@SQ\tSN:<name>\tLN:<len>\n" with len = the next sorted start - this one,
// and n - start for the last (n: the index's text length; 0 if the start lies beyond it).  That is an UPPER BOUND of the sequence's length: it includes
// the separators between documents and the terminator.  Names pair with sorted starts by position, as rbg_doc_table lists them.
#ifndef RBG_SAM_HPP
#define RBG_SAM_HPP
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RBG_SAM_HD __host__ __device__ __forceinline__
#else
#define RBG_SAM_HD inline
#endif

#include <cstdint>
#include <string>
#include <vector>

namespace rbg {

constexpr uint32_t kSamFlagReverse = 16, kSamFlagSecondary = 256, kSamFlagUnmapped = 4;

#ifndef RBG_SAM_MAX_MISMATCH
#define RBG_SAM_MAX_MISMATCH 8
#endif
// what the left extension of one line leaves behind (include/rbg.h rbg_extend_t has the same layout)
struct SamExtend {
    uint32_t ext, nm;                           // e, and the mismatches inside it
    int32_t score;                              // best
    uint32_t steps;                             // bases taken
    uint32_t mis_t[RBG_SAM_MAX_MISMATCH];       // the taken mismatches in the order met: t ...
    uint8_t mis_ref[RBG_SAM_MAX_MISMATCH];      // ... and the reference base c; unused entries are zero
};
static_assert(sizeof(SamExtend) == 56, "four words, eight words, eight bytes");

RBG_SAM_HD bool sam_is_acgt(const uint32_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
// the rule above, one base per call
struct SamExtendWalk {
    uint32_t L, K, t, mm, e, nm, steps;
    int32_t score, best;
};
RBG_SAM_HD SamExtendWalk sam_extend_begin(const uint64_t a, const uint64_t offs, const uint32_t K) {
    return SamExtendWalk{static_cast<uint32_t>(a < offs ? a : offs), K, 0u, 0u, 0u, 0u, 0u, 0, 0};
}
// c = BWT[r] (any value that is not A C G T: stop), x = s[a-1-t].  false: the walk ends here, the base is not taken.  true: the base is taken (the caller
// steps r = LF(r, c)); *mismatch: remember (t, c) as entry mm - 1 -- t is w.t - 1 after the call
RBG_SAM_HD bool sam_extend_take(SamExtendWalk &w, const uint32_t c, const uint32_t x, bool *mismatch) {
    *mismatch = false;
    if (w.t >= w.L || !sam_is_acgt(c)) return false;
    if (c == x) {
        w.score += 1;
    } else {
        if (w.mm + 1 > w.K) return false;
        w.mm += 1;
        w.score -= 4;
        *mismatch = true;
    }
    w.t += 1;
    w.steps += 1;
    if (w.score >= w.best) { w.best = w.score; w.e = w.t; w.nm = w.mm; }
    return true;
}

RBG_SAM_HD uint8_t sam_comp(const uint8_t c) {
    switch (c) {
        case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
        case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a';
        default: return c;
    }
}

// (the same digits as rbg_text_dev.hpp's dec_len / put_dec; restated so that a host compiler needs this header only)
RBG_SAM_HD uint32_t sam_dec_len(uint64_t v) {
    uint32_t n = 1;
    while (v >= 10) { v /= 10; ++n; }
    return n;
}
template <typename Ptr>
RBG_SAM_HD uint32_t sam_put_dec(Ptr p, uint64_t v) {
    const uint32_t n = sam_dec_len(v);
    for (uint32_t j = n; j-- > 0;) {
        const uint64_t q = v / 10;
        p[j] = static_cast<char>('0' + static_cast<uint32_t>(v - q * 10));
        v = q;
    }
    return n;
}

RBG_SAM_HD uint32_t sam_cigar_len(const uint64_t m, const uint64_t a, const uint64_t b) {
    return (a ? sam_dec_len(a) + 1 : 0) + sam_dec_len(b - a) + 1 + (m > b ? sam_dec_len(m - b) + 1 : 0);
}
template <typename Ptr>
RBG_SAM_HD uint32_t sam_put_cigar(Ptr p, const uint64_t m, const uint64_t a, const uint64_t b) {
    uint32_t n = 0;
    if (a) { n += sam_put_dec(p + n, a); p[n++] = 'S'; }
    n += sam_put_dec(p + n, b - a);
    p[n++] = 'M';
    if (m > b) { n += sam_put_dec(p + n, m - b); p[n++] = 'S'; }
    return n;
}

// one line, by its parts
struct SamLine {
    uint64_t name_len;
    bool mapped;
    bool reverse;      // mapped: the seed was found in the reverse complement
    uint64_t hit;      // mapped: 1 = the primary line, j > 1 = the secondary line of location j
    uint64_t occ;      // mapped: hi - lo + 1
    uint64_t rname_len, pos;   // mapped: the document's name, 1 + offset
    uint64_t m, a, b;  // read length; mapped: the seed [a, b) in the searched orientation
    bool has_qual;     // the call has quality bytes
};
RBG_SAM_HD uint32_t sam_flag(const SamLine &L) {
    return L.mapped ? (L.reverse ? kSamFlagReverse : 0u) | (L.hit > 1 ? kSamFlagSecondary : 0u) : kSamFlagUnmapped;
}
RBG_SAM_HD uint64_t sam_seq_len(const SamLine &L) { return (L.mapped && L.hit > 1) || L.m == 0 ? 1 : L.m; }
RBG_SAM_HD uint64_t sam_qual_len(const SamLine &L) { return (L.mapped && L.hit > 1) || L.m == 0 || !L.has_qual ? 1 : L.m; }
constexpr uint32_t kSamUnmappedMid = 17;   // "\t4\t*\t0\t0\t*\t*\t0\t0\t"
// MD:Z: of an extended line: the read positions [a - e, b) from the left, u = e - 1 - t the position of the mismatch met at t.  y (nullable): the line's
// RIGHT extension -- the positions [b, b + y->ext) follow, the mismatch met at t sits t bases right of b; the number around the seed joins both flanks' matches
RBG_SAM_HD uint32_t sam_md_len(const SamExtend *x, const uint64_t seed_len, const SamExtend *y = nullptr) {
    uint32_t n = 0, prev = 0;
    for (uint32_t i = x->nm; i-- > 0;) {
        const uint32_t u = x->ext - 1 - x->mis_t[i];
        n += sam_dec_len(u - prev) + 1;
        prev = u + 1;
    }
    uint64_t run = static_cast<uint64_t>(x->ext - prev) + seed_len;
    if (y) {
        uint32_t at = 0;
        for (uint32_t i = 0; i < y->nm; ++i) {
            n += sam_dec_len(run + (y->mis_t[i] - at)) + 1;
            run = 0;
            at = y->mis_t[i] + 1;
        }
        run += y->ext - at;
    }
    return n + sam_dec_len(run);
}
template <typename Ptr>
RBG_SAM_HD uint32_t sam_put_md(Ptr p, const SamExtend *x, const uint64_t seed_len, const SamExtend *y = nullptr) {
    uint32_t n = 0, prev = 0;
    for (uint32_t i = x->nm; i-- > 0;) {
        const uint32_t u = x->ext - 1 - x->mis_t[i];
        n += sam_put_dec(p + n, u - prev);
        p[n++] = static_cast<char>(x->mis_ref[i]);
        prev = u + 1;
    }
    uint64_t run = static_cast<uint64_t>(x->ext - prev) + seed_len;
    if (y) {
        uint32_t at = 0;
        for (uint32_t i = 0; i < y->nm; ++i) {
            n += sam_put_dec(p + n, run + (y->mis_t[i] - at));
            p[n++] = static_cast<char>(y->mis_ref[i]);
            run = 0;
            at = y->mis_t[i] + 1;
        }
        run += y->ext - at;
    }
    return n + sam_put_dec(p + n, run);
}
// x (nullable): the line's left extension -- POS and the clip move by x->ext, the tags NM, MD and AS follow HI (mapped lines only).  y (nullable, only
// with x): its right extension -- the right clip shrinks by y->ext, NM, MD and AS take both flanks
RBG_SAM_HD uint64_t sam_line_len(const SamLine &L, const SamExtend *x = nullptr, const SamExtend *y = nullptr) {
    if (!L.mapped) return L.name_len + kSamUnmappedMid + sam_seq_len(L) + 1 + sam_qual_len(L) + 1;
    const uint64_t e = x ? x->ext : 0, er = y ? y->ext : 0;
    uint64_t n = L.name_len + 1 + sam_dec_len(sam_flag(L)) + 1 + L.rname_len + 1 + sam_dec_len(L.pos - e) + 5 /* \t255\t */ + sam_cigar_len(L.m, L.a - e, L.b + er) +
                 7 /* \t*\t0\t0\t */ + sam_seq_len(L) + 1 + sam_qual_len(L) + 6 /* \tNH:i: */ + sam_dec_len(L.occ) + 6 /* \tHI:i: */ + sam_dec_len(L.hit) + 1;
    if (x) n += 6 /* \tNM:i: */ + sam_dec_len(x->nm + (y ? y->nm : 0u)) + 6 /* \tMD:Z: */ + sam_md_len(x, L.b - L.a, y) + 6 /* \tAS:i: */ +
                sam_dec_len(L.b - L.a + static_cast<uint64_t>(x->score) + (y ? static_cast<uint64_t>(y->score) : 0));
    return n;
}

template <typename Ptr>
RBG_SAM_HD Ptr sam_put_lit(Ptr p, const char *s, const uint32_t n) {
    for (uint32_t j = 0; j < n; ++j) p[j] = s[j];
    return p + n;
}
// SEQ or QUAL: n = 1 and "*", or the m bytes of src, forwards or backwards, complemented or not
template <typename Ptr>
RBG_SAM_HD Ptr sam_put_bases(Ptr p, const char *src, const uint64_t m, const bool star, const bool backwards, const bool complement) {
    if (star) { p[0] = '*'; return p + 1; }
    for (uint64_t j = 0; j < m; ++j) {
        const uint8_t c = static_cast<uint8_t>(src[backwards ? m - 1 - j : j]);
        p[j] = static_cast<char>(complement ? sam_comp(c) : c);
    }
    return p + m;
}
// the sam_line_len(L, x, y) bytes of the line at p; seq / qual: the read's ORIGINAL bytes (qual unused without has_qual)
template <typename Ptr>
RBG_SAM_HD void sam_put_line(Ptr p, const SamLine &L, const char *name, const char *rname, const char *seq, const char *qual, const SamExtend *x = nullptr,
                             const SamExtend *y = nullptr) {
    for (uint64_t j = 0; j < L.name_len; ++j) p[j] = name[j];
    p += L.name_len;
    const bool star = (L.mapped && L.hit > 1) || L.m == 0;
    if (!L.mapped) {
        p = sam_put_lit(p, "\t4\t*\t0\t0\t*\t*\t0\t0\t", kSamUnmappedMid);
        p = sam_put_bases(p, seq, L.m, star, false, false);
        *p = '\t'; p += 1;
        p = sam_put_bases(p, qual, L.m, star || !L.has_qual, false, false);
        *p = '\n';
        return;
    }
    *p = '\t'; p += 1;
    p += sam_put_dec(p, sam_flag(L));
    *p = '\t'; p += 1;
    for (uint64_t j = 0; j < L.rname_len; ++j) p[j] = rname[j];
    p += L.rname_len;
    *p = '\t'; p += 1;
    const uint64_t e = x ? x->ext : 0, er = y ? y->ext : 0;
    p += sam_put_dec(p, L.pos - e);
    p = sam_put_lit(p, "\t255\t", 5);
    p += sam_put_cigar(p, L.m, L.a - e, L.b + er);
    p = sam_put_lit(p, "\t*\t0\t0\t", 7);
    p = sam_put_bases(p, seq, L.m, star, L.reverse, L.reverse);
    *p = '\t'; p += 1;
    p = sam_put_bases(p, qual, L.m, star || !L.has_qual, L.reverse, false);
    p = sam_put_lit(p, "\tNH:i:", 6);
    p += sam_put_dec(p, L.occ);
    p = sam_put_lit(p, "\tHI:i:", 6);
    p += sam_put_dec(p, L.hit);
    if (x) {
        p = sam_put_lit(p, "\tNM:i:", 6);
        p += sam_put_dec(p, x->nm + (y ? y->nm : 0u));
        p = sam_put_lit(p, "\tMD:Z:", 6);
        p += sam_put_md(p, x, L.b - L.a, y);
        p = sam_put_lit(p, "\tAS:i:", 6);
        p += sam_put_dec(p, L.b - L.a + static_cast<uint64_t>(x->score) + (y ? static_cast<uint64_t>(y->score) : 0));
    }
    *p = '\n';
}

// the header's text (host).  sorted[ndocs]: the documents' starts ascending, names[j] the name listed with sorted[j]; n: the text length of the index
inline std::string sam_header_text(const std::vector<std::string> &names, const std::vector<uint64_t> &sorted, const uint64_t n, const char *pg_line) {
    std::string s = "@HD\tVN:1.6\tSO:unsorted\n";
    for (size_t j = 0; j < sorted.size(); ++j) {
        const uint64_t end = j + 1 < sorted.size() ? sorted[j + 1] : n;
        s += "@SQ\tSN:";
        s += names[j];
        s += "\tLN:";
        s += std::to_string(end > sorted[j] ? end - sorted[j] : 0);
        s += '\n';
    }
    if (pg_line) s += pg_line;
    return s;
}

}  // namespace rbg
#endif
