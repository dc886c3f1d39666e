// The left-extension rules that host and device share (rowbowt_amd/csrc/rbg_sam.hpp), on the host: the walk (sam_extend_begin / sam_extend_take) against a
// direct evaluation over bytes, and sam_line_len / sam_put_line with extension records against lines put together from strings, with sentinels on both
// sides of the buffer.  Stand-alone: g++ -fsanitize=address,undefined tests/cpp/sam_extend_host_check.cpp.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../rowbowt_amd/csrc/rbg_sam.hpp"

using namespace rbg;

static unsigned long long g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

// the walk of the rule over ref (the bases left of the seed, nearest first) and prefix (the read's bases left of the seed, nearest first)
static SamExtend walk(const std::string &ref, const std::string &pre, uint64_t offs, uint32_t K) {
    SamExtend x;
    std::memset(&x, 0, sizeof x);
    SamExtendWalk w = sam_extend_begin(pre.size(), offs, K);
    while (w.t < w.L) {
        const uint32_t c = static_cast<uint8_t>(ref[w.t]), r = static_cast<uint8_t>(pre[w.t]);
        bool mis;
        if (!sam_extend_take(w, c, r, &mis)) break;
        if (mis) { x.mis_t[w.mm - 1] = w.t - 1; x.mis_ref[w.mm - 1] = static_cast<uint8_t>(c); }
    }
    x.ext = w.e; x.nm = w.nm; x.score = w.best; x.steps = w.steps;
    return x;
}

// the same by the pseudo-code, written out again
static SamExtend direct(const std::string &ref, const std::string &pre, uint64_t offs, uint32_t K) {
    SamExtend x;
    std::memset(&x, 0, sizeof x);
    const uint64_t L = pre.size() < offs ? pre.size() : offs;
    int score = 0, best = 0;
    uint32_t mm = 0;
    for (uint64_t t = 0; t < L; ++t) {
        const char c = ref[t];
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T') break;
        if (c == pre[t]) score += 1;
        else {
            if (++mm > K) break;
            score -= 4;
            x.mis_t[mm - 1] = static_cast<uint32_t>(t);
            x.mis_ref[mm - 1] = static_cast<uint8_t>(c);
        }
        if (score >= best) { best = score; x.ext = static_cast<uint32_t>(t + 1); x.nm = mm; }
        x.steps += 1;
    }
    x.score = best;
    return x;
}

static std::string md_string(const SamExtend &x, uint64_t seed_len) {
    std::string s;
    uint32_t run = 0;
    for (uint32_t u = 0; u < x.ext; ++u) {          // read positions a - e + u; the mismatch met at t sits at u = e - 1 - t
        bool hit = false;
        for (uint32_t i = 0; i < x.nm; ++i)
            if (x.ext - 1 - x.mis_t[i] == u) { s += std::to_string(run) + static_cast<char>(x.mis_ref[i]); run = 0; hit = true; }
        if (!hit) ++run;
    }
    return s + std::to_string(run + seed_len);
}

static void check_line(const SamLine &L, const SamExtend *x, const std::string &name, const std::string &rname, const std::string &seq, const std::string &qual) {
    const uint64_t e = x && L.mapped ? x->ext : 0;
    std::string want = name;
    if (!L.mapped) {
        want += "\t4\t*\t0\t0\t*\t*\t0\t0\t" + (L.m ? seq : std::string("*")) + "\t" + (L.m && L.has_qual ? qual : std::string("*")) + "\n";
    } else {
        std::string cig;
        if (L.a - e) cig += std::to_string(L.a - e) + "S";
        cig += std::to_string(L.b - L.a + e) + "M";
        if (L.m > L.b) cig += std::to_string(L.m - L.b) + "S";
        const bool star = L.hit > 1 || L.m == 0;
        std::string sq = seq, ql = qual;
        if (L.reverse) {
            sq.assign(seq.rbegin(), seq.rend());
            for (auto &c : sq) c = static_cast<char>(sam_comp(static_cast<uint8_t>(c)));
            ql.assign(qual.rbegin(), qual.rend());
        }
        want += "\t" + std::to_string(sam_flag(L)) + "\t" + rname + "\t" + std::to_string(L.pos - e) + "\t255\t" + cig + "\t*\t0\t0\t" + (star ? "*" : sq) + "\t" +
                (star || !L.has_qual ? "*" : ql) + "\tNH:i:" + std::to_string(L.occ) + "\tHI:i:" + std::to_string(L.hit);
        if (x) want += "\tNM:i:" + std::to_string(x->nm) + "\tMD:Z:" + md_string(*x, L.b - L.a) + "\tAS:i:" + std::to_string(L.b - L.a + x->score);
        want += "\n";
    }
    const SamExtend *px = L.mapped ? x : nullptr;
    const uint64_t n = sam_line_len(L, px);
    CHECK(n == want.size());
    std::vector<char> buf(n + 32, '#');
    sam_put_line(buf.data() + 16, L, name.data(), rname.data(), seq.data(), qual.data(), px);
    CHECK(std::memcmp(buf.data() + 16, want.data(), n) == 0);
    for (int j = 0; j < 16; ++j) CHECK(buf[j] == '#' && buf[16 + n + j] == '#');
}

int main() {
    static_assert(sizeof(SamExtend) == 56 && RBG_SAM_MAX_MISMATCH == 8, "the record of include/rbg.h");
    // ---- the walk: random flanks, K = 0 .. 8, limits below, at and beyond the prefix, terminators and N in the reference, N and lower case in the read
    unsigned long long seed = 12345;
    auto rnd = [&](unsigned mod) { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return static_cast<unsigned>((seed >> 33) % mod); };
    unsigned met_trim = 0, met_budget = 0, met_base = 0, met_full = 0;
    for (int it = 0; it < 4000; ++it) {
        const unsigned a = rnd(120);
        std::string ref(a + 4, 'A'), pre(a, 'A');
        for (auto &c : ref) c = "ACGT"[rnd(4)];
        for (unsigned t = 0; t < a; ++t) pre[t] = ref[t];
        const unsigned nsub = rnd(12);
        for (unsigned s = 0; s < nsub && a; ++s) { const unsigned t = rnd(a); pre[t] = "ACGTNa"[rnd(6)]; }
        if (it % 7 == 0 && a) ref[rnd(a)] = "\x01N$"[rnd(3)];
        if (it % 11 == 0 && a) { pre[0] = ref[0] == 'A' ? 'C' : 'A'; }                    // a mismatch at the first extended base
        if (it % 13 == 0 && a > 1) { pre[a - 1] = ref[a - 1] == 'A' ? 'C' : 'A'; }        // ... and at the last
        const uint64_t offs = (it % 5 == 0) ? rnd(a + 1) : (it % 5 == 1 ? a : a + rnd(1000));
        for (uint32_t K = 0; K <= 8; ++K) {
            const SamExtend x = walk(ref, pre, offs, K), y = direct(ref, pre, offs, K);
            CHECK(std::memcmp(&x, &y, sizeof x) == 0);
            CHECK(x.ext <= a && x.ext <= offs && x.nm <= K && x.score == static_cast<int>(x.ext) - 5 * static_cast<int>(x.nm) && x.score >= 0);
            CHECK(x.ext == 0 || pre[x.ext - 1] == ref[x.ext - 1]);
            uint32_t taken = 0;
            for (int k = 0; k < 8; ++k) taken += x.mis_ref[k] ? 1 : 0;
            CHECK(taken <= K && taken >= x.nm);
            met_trim += taken > x.nm;
            met_budget += taken == K && x.steps < (a < offs ? a : offs);
            met_full += x.ext == a && a > 0;
            met_base += x.steps < a && x.steps < offs && !sam_is_acgt(static_cast<uint8_t>(ref[x.steps]));
        }
    }
    CHECK(met_trim > 100 && met_budget > 100 && met_full > 100 && met_base > 100);

    // ---- the lines: MD numbers of 1 to 3 digits, mismatches at the first and last extended base, a POS that loses a digit, every K
    const std::string name = "read/1", rname = "hapX";
    unsigned md_digits[4] = {0, 0, 0, 0}, pos_lost = 0;
    for (uint32_t K = 0; K <= 8; ++K)
        for (unsigned a : {0u, 1u, 5u, 9u, 10u, 99u, 100u, 140u, 250u})
            for (unsigned pattern = 0; pattern < 6; ++pattern) {
                std::string ref(a, 'A'), pre(a, 'A');
                for (unsigned t = 0; t < a; ++t) pre[t] = ref[t] = "ACGT"[(t * 7 + a) % 4];
                auto flip = [&](unsigned t) { if (t < a) pre[t] = ref[t] == 'G' ? 'T' : 'G'; };
                if (pattern == 1) flip(0);
                if (pattern == 2) { flip(0); flip(a - 1); }
                if (pattern == 3) for (unsigned t = 9; t < a; t += 12) flip(t);
                if (pattern == 4) { flip(5); flip(6); flip(a / 2); }
                if (pattern == 5) { flip(a > 104 ? 104 : 0); }
                const uint64_t seed_len = pattern % 2 ? 20 : 105;
                const SamExtend x = walk(ref, pre, 100000, K);
                const std::string md = md_string(x, seed_len);
                for (size_t p = 0; p < md.size();) {
                    size_t q = p;
                    while (q < md.size() && md[q] >= '0' && md[q] <= '9') ++q;
                    if (q - p >= 1 && q - p <= 3) md_digits[q - p]++;
                    p = q + 1;
                }
                for (int rev = 0; rev < 2; ++rev)
                    for (int hit = 1; hit <= 2; ++hit)
                        for (int hq = 0; hq < 2; ++hq)
                            for (uint64_t pos : {uint64_t(1) + x.ext, uint64_t(1000), uint64_t(1000) + x.ext, uint64_t(123456789012ull)}) {
                                const uint64_t m = a + seed_len + (pattern % 3);
                                SamLine L{name.size(), true, rev != 0, static_cast<uint64_t>(hit), 7, rname.size(), pos, m, a, a + seed_len, hq != 0};
                                if (pos <= x.ext) continue;
                                std::string seq(m, 'C'), qual(m, 'I');
                                for (uint64_t j = 0; j < m; ++j) { seq[j] = "ACGTNacgt"[(j * 5 + a) % 9]; qual[j] = static_cast<char>(33 + j % 60); }
                                check_line(L, &x, name, rname, seq, qual);
                                check_line(L, nullptr, name, rname, seq, qual);         // rbg_align_sam's line: unchanged by the optional argument
                                pos_lost += std::to_string(pos).size() > std::to_string(pos - x.ext).size();
                            }
            }
    CHECK(md_digits[1] > 50 && md_digits[2] > 50 && md_digits[3] > 50 && pos_lost > 50);
    {   // unmapped lines ignore the record
        SamExtend x;
        std::memset(&x, 0, sizeof x);
        SamLine L{name.size(), false, false, 1, 1, 0, 0, 12, 0, 0, true};
        check_line(L, &x, name, rname, "ACGTNNACGTAC", "IIIIIIIIIIII");
        L.m = 0;
        check_line(L, &x, name, rname, "", "");
    }
    std::printf("sam extend host ok %llu checks\n", g_checks);
    return 0;
}
