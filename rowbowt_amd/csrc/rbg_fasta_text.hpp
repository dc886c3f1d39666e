// rbg_fasta_text.hpp -- the text an index is built over, from a FASTA file (rb_build --fasta).  Plain C++17 over fastx.hpp's scanner (plain or
// gzip input): a host compiler takes it alone (tests/cpp/fasta_text_check.cpp).
//
// Per record: the name is the header up to its first whitespace; the sequence loses its line ends (CR and LF) and is upper-cased (a-z only); every other byte
// stays as it is -- N, IUPAC letters.  The documents are joined by one '#' and the text ends in the byte 0x01; a document starts at its first byte (for an
// empty document: where its separator stands), so starts = cumsum(len + 1) and an empty record gives "##".  Refused with RBG_EFORMAT: a sequence byte <= 0x01,
// a sequence byte '#', a header with an empty name, a file without a record -- and anything that is not FASTA to the scanner, which reads FASTQ as well: a
// record introduced by '@' (a FASTQ file, or a sequence line that begins with '@') and a '+' line behind a sequence (it would open a quality block).
// RBG_EIO: a file that cannot be opened or read.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rbg.h"
#include "fastx.hpp"

namespace rbg_cli {

struct FastaText {
    std::string text;                  // documents joined by '#', then 0x01
    std::vector<std::string> names;
    std::vector<uint64_t> starts;
    // the .docs file: "name start" per line (what rbg_convert_runs_markers / rbg_convert_text take as docs_text)
    std::string docs_text() const {
        std::string s;
        for (size_t d = 0; d < names.size(); ++d) {
            s += names[d];
            s += ' ';
            put_u64(s, starts[d]);
            s += '\n';
        }
        return s;
    }
};

// RBG_OK, RBG_EIO or RBG_EFORMAT; `why` (nullable) gets a line for the user
inline int fasta_text(const char *path, FastaText &out, std::string *why = nullptr) {
    auto fail = [&](int rc, const std::string &msg) {
        if (why) *why = msg;
        return rc;
    };
    out = FastaText();
    gzFile fp = gzopen(path, "r");
    if (!fp) return fail(RBG_EIO, std::string(path) + " cannot be opened");
    FastxReader rd(fp);
    PackedBatch b;
    int rc;
    while ((rc = rd.next(b)) == 0) {
        const size_t d = b.size() - 1;      // (the batch holds this record alone)
        std::string name = b.names.substr(b.name_off[d], b.name_off[d + 1] - b.name_off[d]);
        if (rd.record_char() != '>' || rd.record_had_quality()) {
            gzclose(fp);
            return fail(RBG_EFORMAT, "record " + std::to_string(out.names.size() + 1) + " is not a FASTA record (a line begins with '@' or '+')");
        }
        if (name.empty()) { gzclose(fp); return fail(RBG_EFORMAT, "record " + std::to_string(out.names.size() + 1) + " has an empty name"); }
        if (!out.names.empty()) out.text.push_back('#');
        out.starts.push_back(out.text.size());
        for (size_t i = b.off[d]; i < b.off[d + 1]; ++i) {
            unsigned char c = static_cast<unsigned char>(b.seqs[i]);
            if (c == '\r' || c == '\n') continue;
            if (c >= 'a' && c <= 'z') c = static_cast<unsigned char>(c - 'a' + 'A');
            if (c <= 0x01 || c == '#') {
                gzclose(fp);
                return fail(RBG_EFORMAT, name + " holds the byte " + std::to_string(static_cast<unsigned>(c)) + ", which the text keeps for itself");
            }
            out.text.push_back(static_cast<char>(c));
        }
        out.names.push_back(std::move(name));
        b.clear();
    }
    gzclose(fp);
    if (rc == -3) return fail(RBG_EIO, std::string(path) + " cannot be read");
    if (rc == -2) return fail(RBG_EFORMAT, std::string(path) + " holds a FASTQ record whose quality is cut short");
    if (out.names.empty()) return fail(RBG_EFORMAT, std::string(path) + " holds no record");
    out.text.push_back('\x01');
    return RBG_OK;
}

}  // namespace rbg_cli
