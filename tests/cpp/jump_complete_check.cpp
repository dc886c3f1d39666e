// CPU test of the completeness rule of the jump table (rowbowt_amd/csrc/rbg_jump.h jump_complete_mask / jump_absent_ends) on a host model: the
// words of K1 and of K1 + K2 symbols that occur in a small random text are enumerated by brute force and inserted into host tables laid out as
// k_jump.hip lays them out, under the insert's own skip rule (a toehold in [0xFFFFFFF0, 2^64 - 1) is not expressible).  For every build -- all
// inserted, one word skipped at either level, no table, level 2 declined, a build that stopped early, the switch off -- the mask is what the
// rule says, and wherever it lets an absent key end a read, EVERY word over the alphabet that the table lacks does not occur in the text (so the
// empty range is the answer); where a word was left out, that very word is absent AND occurs, and the mask must not cover its level.
// Prints "jump complete ok <checks>".
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../rowbowt_amd/csrc/rbg_jump.h"

using namespace rbg;

namespace {

uint64_t checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct HostTable {   // nb buckets x two 8-word slots
    uint64_t nb;
    std::vector<uint32_t> w;
    explicit HostTable(uint64_t n) : nb(n), w(n * 16, 0) {}
    void insert(const JumpKey &k, uint32_t lo) {
        uint64_t b = jump_home(jump_hash(k), nb);
        for (uint64_t step = 0; step < nb; ++step) {
            for (uint32_t s = 0; s < 2; ++s) {
                uint32_t *slot = &w[(2 * b + s) * kJumpSlotWords];
                if (slot[7] == kJumpEmptyTag) {
                    for (int i = 0; i < 4; ++i) slot[i] = k.w[i];
                    slot[4] = lo; slot[5] = lo; slot[6] = 0; slot[7] = kJumpFullTag;
                    return;
                }
            }
            b = jump_next(b, nb);
        }
        std::printf("table full\n");
        std::exit(1);
    }
    bool probe(const JumpKey &k, uint32_t v[3]) const {
        auto load = [&](uint64_t b, uint32_t s, uint32_t kw[4], uint32_t vw[4]) {
            const uint32_t *slot = &w[(2 * b + s) * kJumpSlotWords];
            for (int i = 0; i < 4; ++i) { kw[i] = slot[i]; vw[i] = slot[4 + i]; }
        };
        uint32_t buckets = 0;
        return jump_probe(load, nb, k, v, buckets);
    }
};

// the insert's rule for a word's toehold (k_jump.hip k_jump_insert): 2^64 - 1 travels as 0xFFFFFFFF, other values from 0xFFFFFFF0 up do not fit
bool expressible(uint64_t toehold) { return toehold == ~uint64_t(0) || toehold < 0xFFFFFFF0ull; }

struct Word { std::string s; uint32_t name; uint64_t toehold; };   // name: a number only this word has (the kernel's: lo of its range)

// a level as the load sees it: its table (or none) and the counts the rule reads
struct Level {
    HostTable tab{1};
    JumpBuilt built{false, 0, 0};
};

// key of level 1 from a word of K1 symbols (text order): symbol t of the key = the word's symbol K1 - 1 - t
JumpKey key1(const std::string &wd) {
    JumpKey k{{0, 0, 0, 0}};
    for (uint32_t t = 0; t < wd.size(); ++t) jump_key_set(k, t, static_cast<uint32_t>(wd[wd.size() - 1 - t]));
    return k;
}

Level build(const std::vector<Word> &words, bool level2, uint32_t K2, const std::map<std::string, uint32_t> &name1, bool ran_to_the_end, uint64_t stop_after = ~uint64_t(0)) {
    Level L;
    L.tab = HostTable(jump_buckets_for(words.size()));
    L.built.words = words.size();
    uint64_t done = 0;
    for (const Word &wd : words) {
        if (done++ == stop_after) break;                       // (a build that stopped in the middle of its words)
        if (!expressible(wd.toehold)) continue;
        if (!level2) L.tab.insert(key1(wd.s), wd.name);
        else {
            std::vector<uint8_t> codes(wd.s.begin(), wd.s.end());
            L.tab.insert(jump2_key_from_text(codes.data(), K2, name1.at(wd.s.substr(K2))), wd.name);
        }
        ++L.built.inserted;
    }
    L.built.stands = ran_to_the_end;
    return L;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20261021);
    const uint32_t K1 = 16, K2 = 16;
    // a text over four symbols with repeats (a few haplotypes of one base sequence), so that words share prefixes and suffixes
    std::string base(300, 0), text;
    for (auto &c : base) c = static_cast<char>(rng() & 3u);
    for (int h = 0; h < 4; ++h) {
        std::string hap = base;
        for (int v = 0; v < 6; ++v) hap[rng() % hap.size()] = static_cast<char>(rng() & 3u);
        text += hap;
    }
    auto occurring = [&](uint32_t len) {
        std::map<std::string, uint64_t> first;                   // word -> its last occurrence (the toehold's stand-in)
        for (size_t i = 0; i + len <= text.size(); ++i) first[text.substr(i, len)] = i;
        return first;
    };
    const auto occ1 = occurring(K1), occ2 = occurring(K1 + K2);
    std::vector<Word> w1, w2;
    std::map<std::string, uint32_t> name1;
    for (const auto &kv : occ1) { name1[kv.first] = static_cast<uint32_t>(w1.size() + 1); w1.push_back({kv.first, static_cast<uint32_t>(w1.size() + 1), kv.second}); }
    for (const auto &kv : occ2) w2.push_back({kv.first, static_cast<uint32_t>(w2.size() + 1), kv.second});
    CHECK(w1.size() > 300 && w2.size() > 300);

    // queries: every word that occurs, and as many that do not (a word that occurs with one symbol changed, mostly absent)
    auto queries = [&](const std::map<std::string, uint64_t> &occ) {
        std::vector<std::string> q;
        for (const auto &kv : occ) {
            q.push_back(kv.first);
            std::string m = kv.first;
            const size_t at = rng() % m.size();
            m[at] = static_cast<char>((m[at] + 1 + rng() % 3) & 3);
            q.push_back(m);
        }
        return q;
    };
    const auto q1 = queries(occ1), q2 = queries(occ2);

    // what the kernel does with a read whose last K1 (+ K2) symbols are `q`: true = the read was ended at a probe
    auto ended_at_probe = [&](const Level &l1, const Level &l2, uint32_t mask, const std::string &q, bool &wrong) {
        wrong = false;
        uint32_t v[3];
        const std::string tail1 = q.substr(q.size() - K1);
        const bool hit1 = l1.built.stands && l1.tab.probe(key1(tail1), v);
        if (!hit1) {
            if (!l1.built.stands || !jump_absent_ends(mask, 0)) return false;
            wrong = occ1.count(tail1) != 0;                    // ended, but the word occurs
            return true;
        }
        CHECK(v[0] == name1.at(tail1));
        if (q.size() < K1 + K2 || !l2.built.stands) return false;
        std::vector<uint8_t> codes(q.begin(), q.end());
        const bool hit2 = l2.tab.probe(jump2_key_from_text(codes.data(), K2, v[0]), v);
        if (hit2 || !jump_absent_ends(mask, 1)) return false;
        wrong = occ2.count(q) != 0;
        return true;
    };
    auto run = [&](const Level &l1, const Level &l2, bool absent_ends, uint32_t want_mask, uint64_t &ended) {
        const uint32_t mask = jump_complete_mask(l1.built, l2.built, absent_ends);
        CHECK(mask == want_mask);
        ended = 0;
        for (const auto *qs : {&q1, &q2})
            for (const std::string &q : *qs) {
                bool wrong = false;
                if (ended_at_probe(l1, l2, mask, q, wrong)) ++ended;
                CHECK(!wrong);
            }
    };
    uint64_t ended = 0, ended_both = 0;
    const Level none{};                                            // no table: stands = false
    // ---- all inserted: both levels complete; absent keys end reads, never one that occurs
    const Level a1 = build(w1, false, 0, name1, true), a2 = build(w2, true, K2, name1, true);
    CHECK(a1.built.inserted == w1.size() && a2.built.inserted == w2.size());
    run(a1, a2, true, kJumpComplete1 | kJumpComplete2, ended_both);
    CHECK(ended_both > 300);
    // ---- the switch off: nothing ends
    run(a1, a2, false, 0u, ended);
    CHECK(ended == 0);
    // ---- one word of level 1 skipped (its toehold is not expressible): only level 2 counts, and the skipped word -- absent, occurring -- walks on
    for (uint64_t th : {uint64_t(0xFFFFFFF0ull), uint64_t(0xFFFFFFFFull), uint64_t(0x100000000ull), ~uint64_t(0) - 1}) {
        std::vector<Word> s1 = w1;
        s1[s1.size() / 2].toehold = th;
        const Level b1 = build(s1, false, 0, name1, true);
        CHECK(b1.built.inserted + 1 == b1.built.words);
        uint32_t v[3];
        CHECK(!b1.tab.probe(key1(s1[s1.size() / 2].s), v) && occ1.count(s1[s1.size() / 2].s));
        run(b1, a2, true, kJumpComplete2, ended);
        CHECK(ended > 0 && ended < ended_both);
    }
    {   // (2^64 - 1 is expressible: the word's last row is text position 0)
        std::vector<Word> s1 = w1;
        s1[3].toehold = ~uint64_t(0);
        CHECK(build(s1, false, 0, name1, true).built.inserted == w1.size());
    }
    // ---- one word of level 2 skipped: only level 1 counts
    {
        std::vector<Word> s2 = w2;
        s2[s2.size() / 3].toehold = 0xFFFFFFF7ull;
        const Level b2 = build(s2, true, K2, name1, true);
        CHECK(b2.built.inserted + 1 == b2.built.words);
        run(a1, b2, true, kJumpComplete1, ended);
        CHECK(ended > 0 && ended < ended_both);
    }
    // ---- level 2 declined (by the budget, or switched off) while level 1 stands: only level 1 is complete -- whatever the declined build counted
    {
        Level d2 = none;
        d2.built.words = w2.size();                               // (the enumeration ran, the table was not allocated)
        run(a1, d2, true, kJumpComplete1, ended);
        CHECK(ended > 0 && ended < ended_both);
        d2.built.inserted = w2.size();
        run(a1, d2, true, kJumpComplete1, ended);
        run(a1, none, true, kJumpComplete1, ended);
    }
    // ---- no table at all: nothing is complete; a level 2 cannot stand alone
    run(none, none, true, 0u, ended);
    CHECK(ended == 0);
    CHECK(jump_complete_mask(JumpBuilt{false, w1.size(), w1.size()}, a2.built, true) == 0u);
    // ---- a build that stopped before its last word but reports a table: inserted != words, not complete
    {
        const Level h1 = build(w1, false, 0, name1, true, w1.size() - 1);
        CHECK(h1.built.inserted + 1 == h1.built.words);
        run(h1, a2, true, kJumpComplete2, ended);
        // ... and one that inserted everything but did not run to the end (its table is not the index's)
        Level e1 = a1;
        e1.built.stands = false;
        CHECK(jump_complete_mask(e1.built, a2.built, true) == 0u);
    }
    // ---- no word occurs: an empty enumeration completes nothing
    CHECK(!jump_level_complete(JumpBuilt{true, 0, 0}));
    CHECK(jump_absent_ends(3u, 0) && jump_absent_ends(3u, 1) && jump_absent_ends(1u, 0) && !jump_absent_ends(1u, 1) && !jump_absent_ends(2u, 0) && !jump_absent_ends(0u, 0));
    std::printf("jump complete ok %llu\n", static_cast<unsigned long long>(checks));
    return 0;
}
