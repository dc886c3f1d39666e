// rbg_vcf.hpp -- the text and the site records of rb_build --fasta --vcf: a reference FASTA and a VCF of phased single-base variants become
// the haplotype documents an index is built over and one site record per document and site (include/rbg.h: rbg_build_from_text_markers).  Plain C++17 over
// fastx.hpp and rbg_fasta_text.hpp (the VCF plain or gzip, through zlib as the FASTA): a host compiler takes it alone (tests/cpp/vcf_text_check.cpp).
//
// Documents, in order: every contig of the FASTA under its name; then per selected sample, in VCF column order, and per haplotype h of its GT every contig
// with that haplotype's alleles applied, named <sample>.<h + 1>.<contig>.  A sample's haplotypes are as many as its largest ploidy; a contig on which it is
// haploid appears in the first only, a contig without an accepted site in all of them; a sample without any accepted site has no known ploidy and gets no
// documents (no_haplotypes names it).  The text rule is rbg_fasta_text.hpp's ('#' joined, a final 0x01).
// Records: per document and accepted site on its contig (pos = the site in that document, first = max(document start, pos - w + 1), val = allele << 60 |
// contig << 48 | 0-based position; the reference documents carry allele 0), sorted by pos.
// Accepted: REF and every ALT one base of ACGT (either case), REF equal to the reference base, at most 15 ALTs.  Skipped and counted (skipped[]): indels and
// MNVs; symbolic, '*', breakend or non-ACGT alleles; sites on a contig the FASTA lacks; a second site at a position (the first is kept).  GT: '.' is the
// reference allele; '/' between equal alleles is taken, between different ones refused.  RBG_EFORMAT with the line in bad_line and `why`: no #CHROM line,
// fewer than 10 columns (or not as many as the #CHROM line), a REF that disagrees with the FASTA, a named sample that is absent, a POS of 0 or beyond the
// contig, no GT or one that does not parse, a ploidy that changes within a sample and contig, more than 4096 contigs (line 0).  Out of scope: indels, the
// text-keyed .midx of rb_locs, a text that does not fit the device.
#pragma once

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "rbg_fasta_text.hpp"

namespace rbg_cli {

enum { VCF_SKIP_INDEL = 0, VCF_SKIP_SYMBOLIC = 1, VCF_SKIP_CONTIG = 2, VCF_SKIP_DUPLICATE = 3 };

struct VcfText {
    FastaText t;                            // the documents: text, names, starts
    std::vector<uint64_t> pos, first, val;  // the site records, ascending in pos
    uint64_t skipped[4] = {0, 0, 0, 0};
    uint64_t sites = 0, bad_line = 0;
    std::vector<std::string> no_haplotypes;     // selected samples without an accepted site: their ploidy is unknown, they get no documents
};

namespace vcf_detail {
inline std::vector<std::string> split(const std::string &s, const char sep) {
    std::vector<std::string> out;
    size_t a = 0;
    for (;;) {
        const size_t b = s.find(sep, a);
        out.push_back(s.substr(a, b == std::string::npos ? b : b - a));
        if (b == std::string::npos) return out;
        a = b + 1;
    }
}
inline bool acgt(const std::string &s) { return s.size() == 1 && (s[0] == 'A' || s[0] == 'C' || s[0] == 'G' || s[0] == 'T'); }
inline void upper(std::string &s) {
    for (char &c : s)
        if (c >= 'a' && c <= 'z') c = static_cast<char>(c - 'a' + 'A');
}
// digits only, at most 18 of them
inline bool number(const std::string &s, uint64_t &v) {
    if (s.empty() || s.size() > 18) return false;
    v = 0;
    for (const char c : s) {
        if (c < '0' || c > '9') return false;
        v = v * 10 + static_cast<uint64_t>(c - '0');
    }
    return true;
}
// the lines of a plain or gzip file, without their '\n'; closed when it goes
struct GzLines {
    gzFile fp;
    std::vector<char> buf;
    bool bad = false;
    explicit GzLines(const char *path) : fp(gzopen(path, "r")), buf(1 << 16) {}
    GzLines(const GzLines &) = delete;
    GzLines &operator=(const GzLines &) = delete;
    ~GzLines() { if (fp) gzclose(fp); }
    bool next(std::string &line) {
        line.clear();
        bool any = false;
        while (gzgets(fp, buf.data(), static_cast<int>(buf.size()))) {
            any = true;
            line += buf.data();      // (a NUL byte inside a line ends what is taken of this piece: such a line fails its column count)
            if (!line.empty() && line.back() == '\n') {
                line.pop_back();
                return true;
            }
        }
        int err = 0;
        (void)gzerror(fp, &err);
        if (err != Z_OK && err != Z_STREAM_END) bad = true;
        return any && !bad;
    }
};
struct Site {
    std::string alts;                          // one base per ALT
    std::vector<std::vector<uint8_t>> per;     // per selected sample: the allele of every haplotype
};
}  // namespace vcf_detail

// RBG_OK, RBG_EIO or RBG_EFORMAT.  samples: the names to take (nullptr: all); w: the window, 1..64
inline int vcf_text(const char *fasta, const char *vcf, const std::vector<std::string> *samples, const uint32_t w, VcfText &out, std::string *why = nullptr) {
    using namespace vcf_detail;
    out = VcfText();
    auto fail = [&](int rc, uint64_t line, const std::string &msg) {
        out.bad_line = line;
        if (why) *why = line ? "line " + std::to_string(line) + " of " + vcf + ": " + msg : msg;
        return rc;
    };
    if (w < 1 || w > 64) return fail(RBG_EARG, 0, "a window outside 1..64");
    FastaText ref;
    std::string sub;
    int rc = fasta_text(fasta, ref, &sub);
    if (rc) return fail(rc, 0, sub);
    const size_t nc = ref.names.size();
    if (nc > 4096) return fail(RBG_EFORMAT, 0, std::string(fasta) + " holds more than 4096 contigs");
    std::vector<std::string> seqs(nc);
    std::map<std::string, size_t> cidx;
    for (size_t c = 0; c < nc; ++c) {
        const uint64_t end = c + 1 < nc ? ref.starts[c + 1] - 1 : ref.text.size() - 1;
        seqs[c] = ref.text.substr(ref.starts[c], end - ref.starts[c]);
        cidx.emplace(ref.names[c], c);      // (a name held twice: the first contig takes its sites)
    }
    GzLines in(vcf);
    if (!in.fp) return fail(RBG_EIO, 0, std::string(vcf) + " cannot be opened");
    std::vector<std::string> cols;
    std::vector<size_t> chosen;
    std::vector<std::map<uint64_t, Site>> sites(nc);
    std::map<std::pair<size_t, size_t>, size_t> ploidy;      // (sample column, contig)
    uint64_t ln = 0;
    std::string line;
    while (in.next(line)) {      // (one line at a time: a cohort VCF is far larger than what is kept of it)
        ++ln;
        while (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line.compare(0, 2, "##") == 0) continue;
        if (line.compare(0, 6, "#CHROM") == 0) {
            cols = split(line, '\t');
            if (cols.size() < 10) return fail(RBG_EFORMAT, ln, "fewer than 10 columns");
            chosen.clear();
            if (!samples) {
                for (size_t s = 0; s + 9 < cols.size(); ++s) chosen.push_back(s);
            } else {
                std::vector<bool> take(cols.size() - 9, false);
                for (const std::string &name : *samples) {
                    size_t s = 0;
                    while (s + 9 < cols.size() && cols[9 + s] != name) ++s;
                    if (s + 9 == cols.size()) return fail(RBG_EFORMAT, ln, "sample " + name + " is absent");
                    take[s] = true;
                }
                for (size_t s = 0; s < take.size(); ++s)
                    if (take[s]) chosen.push_back(s);
            }
            continue;
        }
        if (line[0] == '#') continue;
        if (cols.empty()) return fail(RBG_EFORMAT, ln, "no #CHROM line before the first record");
        const std::vector<std::string> f = split(line, '\t');
        if (f.size() < 10 || f.size() != cols.size()) return fail(RBG_EFORMAT, ln, "fewer than 10 columns, or not as many as the #CHROM line");
        const auto ci = cidx.find(f[0]);
        if (ci == cidx.end()) { ++out.skipped[VCF_SKIP_CONTIG]; continue; }
        const size_t c = ci->second;
        uint64_t p1 = 0;
        if (!number(f[1], p1) || p1 == 0 || p1 > seqs[c].size()) return fail(RBG_EFORMAT, ln, "POS " + f[1] + " is 0 or beyond " + f[0]);
        const uint64_t p0 = p1 - 1;
        std::string refa = f[3];
        upper(refa);
        std::vector<std::string> alts = split(f[4], ',');
        bool symbolic = false, longer = refa.size() != 1, other = !acgt(refa) || alts.size() > 15;
        for (std::string &x : alts) {
            upper(x);
            if ((!x.empty() && x[0] == '<') || x == "*" || x.find('[') != std::string::npos || x.find(']') != std::string::npos) symbolic = true;
            if (x.size() != 1) longer = true;
            if (!acgt(x)) other = true;
        }
        if (symbolic) { ++out.skipped[VCF_SKIP_SYMBOLIC]; continue; }
        if (longer) { ++out.skipped[VCF_SKIP_INDEL]; continue; }
        if (other) { ++out.skipped[VCF_SKIP_SYMBOLIC]; continue; }
        if (seqs[c][p0] != refa[0]) return fail(RBG_EFORMAT, ln, "REF " + refa + " is not the base of " + f[0] + " at " + f[1]);
        if (sites[c].count(p0)) { ++out.skipped[VCF_SKIP_DUPLICATE]; continue; }
        const std::vector<std::string> fmt = split(f[8], ':');
        size_t gi = 0;
        while (gi < fmt.size() && fmt[gi] != "GT") ++gi;
        if (gi == fmt.size()) return fail(RBG_EFORMAT, ln, "no GT in FORMAT");
        Site site;
        for (const std::string &x : alts) site.alts.push_back(x[0]);
        for (const size_t s : chosen) {
            const std::vector<std::string> sf = split(f[9 + s], ':');
            if (gi >= sf.size()) return fail(RBG_EFORMAT, ln, "no GT for sample " + cols[9 + s]);
            const std::string &gt = sf[gi];
            std::vector<uint8_t> al;
            bool unphased = false;
            size_t from = 0;
            for (size_t k = 0; k <= gt.size(); ++k) {
                if (k < gt.size() && gt[k] != '|' && gt[k] != '/') continue;
                if (k < gt.size() && gt[k] == '/') unphased = true;
                const std::string tok = gt.substr(from, k - from);
                from = k + 1;
                uint64_t v = 0;
                if (tok == ".") v = 0;
                else if (!number(tok, v) || v > alts.size()) return fail(RBG_EFORMAT, ln, "GT " + gt + " of sample " + cols[9 + s] + " does not parse");
                al.push_back(static_cast<uint8_t>(v));
            }
            if (unphased)
                for (const uint8_t v : al)
                    if (v != al[0]) return fail(RBG_EFORMAT, ln, "GT " + gt + " of sample " + cols[9 + s] + " is unphased: its haplotypes are undefined");
            const auto pl = ploidy.emplace(std::make_pair(s, c), al.size());
            if (pl.first->second != al.size()) return fail(RBG_EFORMAT, ln, "the ploidy of sample " + cols[9 + s] + " changes on " + f[0]);
            site.per.push_back(std::move(al));
        }
        sites[c].emplace(p0, std::move(site));
        ++out.sites;
    }
    if (in.bad) return fail(RBG_EIO, 0, std::string(vcf) + " cannot be read");
    if (cols.empty()) return fail(RBG_EFORMAT, ln + 1, "no #CHROM line");

    struct Rec { uint64_t pos, first, val; };
    std::vector<Rec> recs;
    FastaText &t = out.t;
    auto add_doc = [&](const std::string &name, const size_t c, const long k /* selected sample, -1: the reference */, const size_t h) {
        if (!t.names.empty()) t.text.push_back('#');
        const uint64_t start = t.text.size();
        t.starts.push_back(start);
        t.names.push_back(name);
        t.text += seqs[c];
        for (const auto &kv : sites[c]) {
            const uint64_t a = k < 0 ? 0 : kv.second.per[static_cast<size_t>(k)][h], p = start + kv.first;
            if (a) t.text[p] = kv.second.alts[a - 1];
            recs.push_back({p, kv.first + 1 >= w ? p - (w - 1) : start, (a << 60) | (static_cast<uint64_t>(c) << 48) | kv.first});
        }
    };
    for (size_t c = 0; c < nc; ++c) add_doc(ref.names[c], c, -1, 0);
    for (size_t k = 0; k < chosen.size(); ++k) {
        const size_t s = chosen[k];
        size_t nhap = 0;
        for (size_t c = 0; c < nc; ++c) {
            const auto it = ploidy.find(std::make_pair(s, c));
            if (it != ploidy.end()) nhap = std::max(nhap, it->second);
        }
        if (nhap == 0) out.no_haplotypes.push_back(cols[9 + s]);
        for (size_t h = 0; h < nhap; ++h)
            for (size_t c = 0; c < nc; ++c) {
                const auto it = ploidy.find(std::make_pair(s, c));
                if ((it == ploidy.end() ? nhap : it->second) <= h) continue;
                add_doc(cols[9 + s] + "." + std::to_string(h + 1) + "." + ref.names[c], c, static_cast<long>(k), h);
            }
    }
    t.text.push_back('\x01');
    // (documents are appended in text order and a document's sites ascend: the records are sorted by pos already)
    out.pos.reserve(recs.size()), out.first.reserve(recs.size()), out.val.reserve(recs.size());
    for (const Rec &r : recs) out.pos.push_back(r.pos), out.first.push_back(r.first), out.val.push_back(r.val);
    return RBG_OK;
}

}  // namespace rbg_cli
