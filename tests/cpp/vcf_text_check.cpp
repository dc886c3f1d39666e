// vcf_text_check <ref.fa> <calls.vcf> <w> [sample,sample,...] -- rbg_vcf.hpp in a program of its own (tests/test_vcf_text_host.py builds it with
// AddressSanitizer and UBSan): prints rc, the line a refusal names, the text and the .docs text as hex, the site records and the skip counts.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../rowbowt_amd/csrc/rbg_vcf.hpp"

static void hex(const char *key, const std::string &s) {
    std::printf("%s=", key);
    for (const unsigned char c : s) std::printf("%02x", c);
    std::printf("\n");
}

static void list(const char *key, const std::vector<uint64_t> &v) {
    std::printf("%s=", key);
    for (size_t i = 0; i < v.size(); ++i) std::printf(i ? ",%llu" : "%llu", static_cast<unsigned long long>(v[i]));
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    std::vector<std::string> samples;
    if (argc > 4) {
        const std::string csv = argv[4];
        for (size_t a = 0; a <= csv.size();) {
            size_t b = csv.find(',', a);
            if (b == std::string::npos) b = csv.size();
            samples.push_back(csv.substr(a, b - a));
            a = b + 1;
        }
    }
    rbg_cli::VcfText v;
    std::string why;
    const int rc = rbg_cli::vcf_text(argv[1], argv[2], argc > 4 ? &samples : nullptr, static_cast<uint32_t>(std::atoi(argv[3])), v, &why);
    std::printf("rc=%d\nline=%llu\nwhy=%s\n", rc, static_cast<unsigned long long>(v.bad_line), why.c_str());
    if (rc) return 0;
    hex("text", v.t.text);
    hex("docs", v.t.docs_text());
    list("pos", v.pos);
    list("first", v.first);
    list("val", v.val);
    std::printf("skipped=%llu,%llu,%llu,%llu\n", static_cast<unsigned long long>(v.skipped[0]), static_cast<unsigned long long>(v.skipped[1]),
                static_cast<unsigned long long>(v.skipped[2]), static_cast<unsigned long long>(v.skipped[3]));
    return 0;
}
