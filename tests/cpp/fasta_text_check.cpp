// The text rule of rb_build --fasta (rowbowt_amd/csrc/rbg_fasta_text.hpp) in a program of its own: fasta_text_check <file> prints the return code, then the
// text and the .docs text as hex.  tests/test_fasta_text_host.py builds it with -fsanitize=address,undefined and compares it with a Python model of the rule.
#include <cstdio>
#include <string>

#include "../../rowbowt_amd/csrc/rbg_fasta_text.hpp"

static void hex(const char *what, const std::string &s) {
    std::printf("%s=", what);
    for (unsigned char c : s) std::printf("%02x", c);
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    rbg_cli::FastaText t;
    std::string why;
    const int rc = rbg_cli::fasta_text(argv[1], t, &why);
    std::printf("rc=%d\n", rc);
    if (rc) {
        std::printf("why=%s\n", why.c_str());
        return 0;
    }
    hex("text", t.text);
    hex("docs", t.docs_text());
    std::printf("ndocs=%zu\n", t.names.size());
    return 0;
}
