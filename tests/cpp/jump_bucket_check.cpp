// CPU test of jump_bucket and of jump_probe re-expressed over it (rowbowt_amd/csrc/rbg_jump.h) on host-built tables of nb = 1, 2, 3 and 8
// buckets: every answer -- hit or absent, the values, the number of buckets read -- is checked against a linear scan of the table that
// follows the probe order by itself (slot 0, slot 1, next bucket, wrapping, at most nb buckets).  Covered by construction: chains that wrap
// from bucket nb - 1 to 0, a key in slot 1 behind a different key in slot 0, an absent key whose chain ends at an empty slot 1, an absent key
// in a table with no empty slot (the nb-bucket bound).  Prints "jump bucket ok <checks>".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../rowbowt_amd/csrc/rbg_jump.h"

using namespace rbg;

namespace {

bool same(const uint32_t *slot, const JumpKey &k) { return slot[0] == k.w[0] && slot[1] == k.w[1] && slot[2] == k.w[2] && slot[3] == k.w[3]; }

struct HostTable {   // nb buckets x two 8-word slots, as k_jump.hip lays them out
    uint64_t nb;
    std::vector<uint32_t> w;
    explicit HostTable(uint64_t n) : nb(n), w(n * 16, 0) {}
    uint32_t *slot(uint64_t b, uint32_t s) { return &w[(2 * b + s) * kJumpSlotWords]; }
    const uint32_t *slot(uint64_t b, uint32_t s) const { return &w[(2 * b + s) * kJumpSlotWords]; }
    void put(uint64_t b, uint32_t s, const JumpKey &k, uint32_t lo, uint32_t hi, uint32_t toe) {
        uint32_t *sl = slot(b, s);
        for (int i = 0; i < 4; ++i) sl[i] = k.w[i];
        sl[4] = lo; sl[5] = hi; sl[6] = toe; sl[7] = kJumpFullTag;
    }
    // k_jump_insert: the first empty slot from `home` on, wrapping; false if the table is full
    bool insert_from(uint64_t home, const JumpKey &k, uint32_t lo, uint32_t hi, uint32_t toe) {
        uint64_t b = home;
        for (uint64_t step = 0; step < nb; ++step) {
            for (uint32_t s = 0; s < 2; ++s)
                if (slot(b, s)[7] == kJumpEmptyTag) { put(b, s, k, lo, hi, toe); return true; }
            b = b + 1 == nb ? 0 : b + 1;
        }
        return false;
    }
    bool insert(const JumpKey &k, uint32_t lo, uint32_t hi, uint32_t toe) { return insert_from(jump_home(jump_hash(k), nb), k, lo, hi, toe); }
    bool probe(const JumpKey &k, uint32_t v[3], uint32_t &buckets) const {
        auto load = [&](uint64_t b, uint32_t s, uint32_t kw[4], uint32_t vw[4]) {
            const uint32_t *sl = slot(b, s);
            for (int i = 0; i < 4; ++i) { kw[i] = sl[i]; vw[i] = sl[4 + i]; }
        };
        buckets = 0;
        return jump_probe(load, nb, k, v, buckets);
    }
    // the linear scan: slot after slot from the home bucket in the probe's order, written without jump_bucket / jump_next
    bool scan(const JumpKey &k, uint32_t v[3], uint32_t &buckets) const {
        const uint64_t home = jump_home(jump_hash(k), nb);
        for (uint64_t t = 0; t < 2 * nb; ++t) {
            const uint32_t *sl = slot((home + t / 2) % nb, static_cast<uint32_t>(t & 1u));
            buckets = static_cast<uint32_t>(t / 2 + 1);
            if (sl[7] == kJumpEmptyTag) return false;
            if (same(sl, k)) { v[0] = sl[4]; v[1] = sl[5]; v[2] = sl[6]; return true; }
        }
        return false;
    }
};

JumpKey random_key(std::mt19937_64 &rng, uint32_t K) {
    JumpKey k{{0, 0, 0, 0}};
    for (uint32_t t = 0; t < K; ++t) jump_key_set(k, t, static_cast<uint32_t>(rng() & 3u));
    return k;
}

JumpKey key_with_home(std::mt19937_64 &rng, uint32_t K, uint64_t nb, uint64_t home) {
    for (;;) {
        const JumpKey k = random_key(rng, K);
        if (jump_home(jump_hash(k), nb) == home) return k;
    }
}

int fail(const char *what, uint64_t nb) {
    std::printf("FAIL: %s (nb = %llu)\n", what, static_cast<unsigned long long>(nb));
    return 1;
}

// jump_probe against the scan, and jump_bucket bucket by bucket along the same chain
int check_key(const HostTable &T, const JumpKey &k, uint64_t &checks) {
    uint32_t v[3] = {~0u, ~0u, ~0u}, sv[3] = {~0u, ~0u, ~0u}, nbk = 0, snbk = 0;
    const bool got = T.probe(k, v, nbk), want = T.scan(k, sv, snbk);
    if (got != want) return fail("jump_probe and the linear scan disagree on hit / absent", T.nb);
    if (nbk != snbk) return fail("jump_probe read another number of buckets than the scan", T.nb);
    if (got && (v[0] != sv[0] || v[1] != sv[1] || v[2] != sv[2])) return fail("jump_probe returned another slot's values", T.nb);
    uint64_t b = jump_home(jump_hash(k), T.nb);
    for (uint32_t step = 1;; ++step) {
        uint32_t bv[3] = {~0u, ~0u, ~0u};
        const uint32_t r = jump_bucket(&T.w[b * 16], k, bv);
        const uint32_t *s0 = T.slot(b, 0), *s1 = T.slot(b, 1);
        const uint32_t expect = s0[7] == kJumpEmptyTag ? kJumpAbsent : same(s0, k) ? kJumpHit0 : s1[7] == kJumpEmptyTag ? kJumpAbsent : same(s1, k) ? kJumpHit1 : kJumpNext;
        if (r != expect) return fail("jump_bucket decided a bucket wrongly", T.nb);
        if (r <= kJumpHit1) {
            const uint32_t *sl = T.slot(b, r);
            if (bv[0] != sl[4] || bv[1] != sl[5] || bv[2] != sl[6]) return fail("jump_bucket filled v from the wrong slot", T.nb);
        } else if (bv[0] != ~0u || bv[1] != ~0u || bv[2] != ~0u) return fail("jump_bucket touched v without a hit", T.nb);
        if (r != kJumpNext) {
            if (step != snbk || (r != kJumpAbsent) != want) return fail("the chain of jump_bucket ends elsewhere than the scan", T.nb);
            break;
        }
        if (step == T.nb) {
            if (want || snbk != T.nb) return fail("a chain of nb full buckets must be an absent key", T.nb);
            break;
        }
        b = jump_next(b, T.nb);
    }
    ++checks;
    return 0;
}

}  // namespace

int main() {
    std::mt19937_64 rng(808);
    uint64_t checks = 0;
    for (uint64_t nb : {1u, 2u, 3u, 8u}) {
        for (uint32_t K : {16u, 60u, 64u}) {
            // (a) a chain from the last bucket that wraps to bucket 0: 2 slots in bucket nb - 1, then as many as fit short of a full table
            {
                HostTable T(nb);
                const uint64_t home = nb - 1;
                const uint32_t nkeys = nb == 1 ? 1u : 3u;             // nb = 1: one key and an empty slot 1; else slot 0 of bucket 0 too
                std::vector<JumpKey> ks;
                for (uint32_t i = 0; i <= nkeys; ++i) ks.push_back(key_with_home(rng, K, nb, home));
                for (uint32_t i = 0; i < nkeys; ++i)
                    if (!T.insert(ks[i], 10 + i, 20 + i, i == 1 ? 0xFFFFFFFFu : 30 + i)) return fail("insert", nb);
                if (nb > 1 && (T.slot(0, 0)[7] != kJumpFullTag || !same(T.slot(0, 0), ks[2]))) return fail("the chain did not wrap to bucket 0", nb);
                for (uint32_t i = 0; i < nkeys; ++i) {
                    uint32_t v[3], n = 0;
                    if (!T.probe(ks[i], v, n) || v[0] != 10 + i || v[1] != 20 + i || n != i / 2 + 1) return fail("key of a wrapping chain", nb);
                    if (check_key(T, ks[i], checks)) return 1;
                }
                // the absent key of the same home: its chain ends at the empty slot 1 (of bucket 0, or of the only bucket)
                uint32_t v[3], n = 0;
                if (T.probe(ks[nkeys], v, n) || n != (nb == 1 ? 1u : 2u)) return fail("absent key ending at an empty slot 1", nb);
                if (check_key(T, ks[nkeys], checks)) return 1;
            }
            // (b) slot 1 behind a different key in slot 0, same home; and an absent third key: continue (nb > 1) into an empty bucket
            {
                HostTable T(nb);
                const uint64_t home = nb / 2;
                const JumpKey a = key_with_home(rng, K, nb, home), b = key_with_home(rng, K, nb, home), c = key_with_home(rng, K, nb, home);
                T.insert(a, 1, 2, 3);
                T.insert(b, 4, 5, 6);
                uint32_t v[3], n = 0, bv[3];
                if (jump_bucket(&T.w[home * 16], b, bv) != kJumpHit1 || bv[0] != 4 || bv[1] != 5 || bv[2] != 6) return fail("slot 1 behind another key", nb);
                if (jump_bucket(&T.w[home * 16], a, bv) != kJumpHit0 || bv[0] != 1) return fail("slot 0", nb);
                if (jump_bucket(&T.w[home * 16], c, bv) != kJumpNext) return fail("a full bucket of other keys must say continue", nb);
                if (!T.probe(b, v, n) || v[0] != 4 || n != 1) return fail("probe of slot 1", nb);
                if (T.probe(c, v, n) || n != (nb == 1 ? 1u : 2u)) return fail("absent key behind a full bucket", nb);
                for (const JumpKey &k : {a, b, c})
                    if (check_key(T, k, checks)) return 1;
            }
            // (c) no empty slot at all: every key found wherever it went, absent keys refused after exactly nb buckets
            {
                HostTable T(nb);
                std::vector<JumpKey> ks;
                for (uint64_t i = 0; i < 2 * nb; ++i) {
                    ks.push_back(random_key(rng, K));
                    if (!T.insert(ks.back(), static_cast<uint32_t>(i), static_cast<uint32_t>(i + 100), static_cast<uint32_t>(i + 200))) return fail("insert into a table with room", nb);
                }
                if (T.insert(random_key(rng, K), 0, 0, 0)) return fail("insert into a full table", nb);
                for (uint64_t i = 0; i < 2 * nb; ++i) {
                    uint32_t v[3], n = 0;
                    if (!T.probe(ks[i], v, n) || v[0] != i || v[1] != i + 100 || v[2] != i + 200) return fail("key of a full table", nb);
                    if (check_key(T, ks[i], checks)) return 1;
                }
                for (int rep = 0; rep < 50; ++rep) {
                    const JumpKey k = random_key(rng, K);
                    uint32_t v[3], n = 0;
                    if (T.probe(k, v, n) || n != nb) return fail("absent key of a full table: the nb-bucket bound", nb);
                    if (check_key(T, k, checks)) return 1;
                }
            }
            // (d) random fill at every load from one key to full, present and absent keys against the scan
            for (uint64_t nkeys = 1; nkeys <= 2 * nb; ++nkeys) {
                HostTable T(nb);
                std::vector<JumpKey> ks;
                for (uint64_t i = 0; i < nkeys; ++i) { ks.push_back(random_key(rng, K)); T.insert(ks.back(), static_cast<uint32_t>(7 * i), static_cast<uint32_t>(7 * i + 1), 0xFFFFFFFFu); }
                for (const JumpKey &k : ks)
                    if (check_key(T, k, checks)) return 1;
                for (int rep = 0; rep < 20; ++rep)
                    if (check_key(T, random_key(rng, K), checks)) return 1;
            }
        }
    }
    std::printf("jump bucket ok %llu\n", static_cast<unsigned long long>(checks));
    return 0;
}
