// CPU test of level 2 of the jump table (rowbowt_amd/csrc/rbg_jump.h) on a host model: the key {the K2 symbols after the first K1, the
// parent range's lo} formed from a staged-code model (words of sixteen 2-bit codes in consumption order, as the search kernel holds a read)
// and from a text word, masking from bit 2 K2 up, the probe against a linear scan on tables of 1, 2, 3 and 8 buckets, and two words of
// equal symbols under different parents.  Prints "jump2 ok <checks>".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../rowbowt_amd/csrc/rbg_jump.h"

using namespace rbg;

namespace {

uint64_t checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

bool same(const JumpKey &a, const JumpKey &b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3]; }

// a read's symbols in consumption order as the staging holds them: word j = symbols [16 j, 16 j + 16), the words after the read garbage
struct Staged {
    std::vector<uint32_t> w;
    Staged(const std::vector<uint8_t> &cons, uint32_t garbage) : w(cons.size() / 16 + 6, garbage) {
        for (size_t t = 0; t < cons.size(); ++t) {
            w[t >> 4] &= ~(3u << (2 * (t & 15)));
            w[t >> 4] |= static_cast<uint32_t>(cons[t] & 3u) << (2 * (t & 15));
        }
    }
    uint32_t operator()(uint32_t j) const { if (j >= w.size()) { std::printf("word %u out of the staging\n", j); std::exit(1); } return w[j]; }
};

struct HostTable {   // nb buckets x two 8-word slots, as k_jump.hip lays them out
    uint64_t nb;
    std::vector<uint32_t> w;
    std::vector<JumpKey> keys;
    std::vector<uint32_t> vals;
    explicit HostTable(uint64_t n) : nb(n), w(n * 16, 0) {}
    bool insert(const JumpKey &k, uint32_t v) {
        uint64_t b = jump_home(jump_hash(k), nb);
        for (uint64_t step = 0; step < nb; ++step) {
            for (uint32_t s = 0; s < 2; ++s) {
                uint32_t *slot = &w[(2 * b + s) * kJumpSlotWords];
                if (slot[7] == kJumpEmptyTag) {
                    for (int i = 0; i < 4; ++i) slot[i] = k.w[i];
                    slot[4] = v; slot[5] = v + 1; slot[6] = v + 2; slot[7] = kJumpFullTag;
                    keys.push_back(k); vals.push_back(v);
                    return true;
                }
            }
            b = jump_next(b, nb);
        }
        return false;
    }
    bool probe(const JumpKey &k, uint32_t v[3]) const {
        auto load = [&](uint64_t b, uint32_t s, uint32_t kw[4], uint32_t vw[4]) {
            const uint32_t *slot = &w[(2 * b + s) * kJumpSlotWords];
            for (int i = 0; i < 4; ++i) { kw[i] = slot[i]; vw[i] = slot[4 + i]; }
        };
        uint32_t buckets = 0;
        const bool hit = jump_probe(load, nb, k, v, buckets);
        CHECK(buckets >= 1 && buckets <= nb);
        return hit;
    }
    bool scan(const JumpKey &k, uint32_t &v) const {
        for (size_t i = 0; i < keys.size(); ++i)
            if (same(keys[i], k)) { v = vals[i]; return true; }
        return false;
    }
};

}  // namespace

int main() {
    std::mt19937_64 rng(20261021);
    const uint32_t K2s[] = {16, 17, 31, 32, 33, 47, 48};
    const uint32_t los[] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu};
    const uint32_t K1s[] = {16, 20, 33, 47, 60, 63, 64};
    // ---- the key from the staged codes, from the text word and symbol by symbol agree; nothing above 2 K2 bits survives
    for (uint32_t K1 : K1s)
        for (uint32_t K2 : K2s)
            for (uint32_t lo : los)
                for (uint32_t extra : {0u, 1u, 9u, 30u}) {
                    const uint32_t m = K1 + K2 + extra;
                    std::vector<uint8_t> text(m);                                   // the read as text, left to right
                    for (auto &c : text) c = static_cast<uint8_t>(rng() & 3u);
                    std::vector<uint8_t> cons(text.rbegin(), text.rend());          // consumption order: last symbol first
                    for (uint32_t garbage : {0u, 0xFFFFFFFFu, 0xA5A5A5A5u}) {
                        const Staged st(cons, garbage);
                        const JumpKey k = jump2_key_from_codes(st, K1, K2, lo);
                        JumpKey want{{0, 0, 0, 0}};
                        for (uint32_t t = 0; t < K2; ++t) jump_key_set(want, t, cons[K1 + t]);
                        want.w[3] = lo;
                        CHECK(same(k, want));
                        // the (K1 + K2)-symbol word as text: the K2 symbols to the left of the K1-mer
                        const JumpKey kt = jump2_key_from_text(text.data() + extra, K2, lo);
                        CHECK(same(kt, want));
                        // masking: bits from 2 K2 up of the symbol words are zero, whatever follows in the read or the staging
                        for (uint32_t b = 2 * K2; b < 96; ++b) CHECK(((k.w[b >> 5] >> (b & 31)) & 1u) == 0);
                        CHECK(k.w[3] == lo);
                        // level 1 through the same helper: the first K1 symbols
                        const JumpKey k1 = jump_key_from_codes(st, 0, K1);
                        JumpKey want1{{0, 0, 0, 0}};
                        for (uint32_t t = 0; t < K1; ++t) jump_key_set(want1, t, cons[t]);
                        CHECK(same(k1, want1));
                    }
                    // jump2_key masks words of symbols given whole
                    const JumpKey km = jump2_key(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, K2, lo);
                    JumpKey ones{{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0}};
                    jump_key_mask(ones, K2);
                    ones.w[3] = lo;
                    CHECK(same(km, ones));
                }
    // ---- equal symbols, different parents: two keys, told apart by the probe
    for (uint32_t K2 : K2s) {
        std::vector<uint8_t> cons(64 + K2);
        for (auto &c : cons) c = static_cast<uint8_t>(rng() & 3u);
        const Staged st(cons, 0);
        HostTable T(2);
        const uint32_t parents[] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu};
        for (uint32_t p : parents) CHECK(T.insert(jump2_key_from_codes(st, 64, K2, p), p ^ 0x1234u));
        for (uint32_t p : parents) {
            uint32_t v[3];
            CHECK(T.probe(jump2_key_from_codes(st, 64, K2, p), v) && v[0] == (p ^ 0x1234u) && v[1] == v[0] + 1 && v[2] == v[0] + 2);
        }
        uint32_t v[3];
        // (a table that is full and lacks the key ends after its nb buckets; one with an empty slot ends there)
        CHECK(!T.probe(jump2_key_from_codes(st, 64, K2, 2u), v));
    }
    // ---- the probe against a linear scan: tables of 1, 2, 3 and 8 buckets at every fill from empty to full
    for (uint64_t nb : {1u, 2u, 3u, 8u})
        for (uint32_t K2 : K2s)
            for (uint64_t fill = 0; fill <= 2 * nb; ++fill) {
                HostTable T(nb);
                std::vector<JumpKey> pool;
                for (uint64_t i = 0; i < 2 * nb + 6; ++i) {
                    JumpKey k = jump2_key(static_cast<uint32_t>(rng()), static_cast<uint32_t>(rng()), static_cast<uint32_t>(rng()), K2, los[rng() & 3u]);
                    if (i & 1u && !pool.empty()) { k = pool[rng() % pool.size()]; k.w[3] ^= 1u << (rng() % 32); }   // same symbols, another parent
                    bool dup = false;
                    for (const JumpKey &q : pool) dup = dup || same(q, k);
                    if (!dup) pool.push_back(k);
                }
                for (uint64_t i = 0; i < fill && i < pool.size(); ++i) CHECK(T.insert(pool[i], static_cast<uint32_t>(i * 3)));
                for (const JumpKey &k : pool) {
                    uint32_t v[3] = {0, 0, 0}, want = 0;
                    const bool in = T.scan(k, want);
                    CHECK(T.probe(k, v) == in);
                    if (in) CHECK(v[0] == want && v[1] == want + 1 && v[2] == want + 2);
                }
            }
    std::printf("jump2 ok %llu\n", static_cast<unsigned long long>(checks));
    return 0;
}
