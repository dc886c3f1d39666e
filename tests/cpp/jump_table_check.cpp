// CPU test of rowbowt_amd/csrc/rbg_jump.h on a host model of the jump table (the device kernels insert and probe with the same
// functions): the key of a read's last K symbols against the 2-bit layout of the packed / staged reads (rbg_pack2bit.hpp), masking
// of what lies beyond K, and probe termination -- a full chain of buckets, a chain that wraps at the table's end, an absent key
// that shares the home bucket, and keys that differ only in their last symbol.  Prints "jump table ok <checks>".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../rowbowt_amd/csrc/rbg_jump.h"
#include "../../rowbowt_amd/csrc/rbg_pack2bit.hpp"

using namespace rbg;

namespace {

struct HostTable {   // nb buckets x two 8-word slots, as k_jump.hip lays them out
    uint64_t nb;
    std::vector<uint32_t> w;
    explicit HostTable(uint64_t n) : nb(n), w(n * 16, 0) {}
    // k_jump_insert: the first empty slot from the home bucket on, wrapping; returns the bucket it went to
    uint64_t insert(const JumpKey &k, uint32_t lo, uint32_t hi, uint32_t toe) {
        uint64_t b = jump_home(jump_hash(k), nb);
        for (uint64_t step = 0; step < nb; ++step) {
            for (uint32_t s = 0; s < 2; ++s) {
                uint32_t *slot = &w[(2 * b + s) * kJumpSlotWords];
                if (slot[7] == kJumpEmptyTag) {
                    for (int i = 0; i < 4; ++i) slot[i] = k.w[i];
                    slot[4] = lo; slot[5] = hi; slot[6] = toe; slot[7] = kJumpFullTag;
                    return b;
                }
            }
            b = b + 1 == nb ? 0 : b + 1;
        }
        std::printf("table full\n");
        std::exit(1);
    }
    bool probe(const JumpKey &k, uint32_t v[3], uint32_t &buckets) const {
        auto load = [&](uint64_t b, uint32_t s, uint32_t kw[4], uint32_t vw[4]) {
            const uint32_t *slot = &w[(2 * b + s) * kJumpSlotWords];
            for (int i = 0; i < 4; ++i) { kw[i] = slot[i]; vw[i] = slot[4 + i]; }
        };
        buckets = 0;
        return jump_probe(load, nb, k, v, buckets);
    }
};

JumpKey key_of(const std::vector<uint8_t> &codes_consumption, uint32_t K) {
    JumpKey k{{0, 0, 0, 0}};
    for (uint32_t t = 0; t < K; ++t) jump_key_set(k, t, codes_consumption[t]);
    return k;
}

JumpKey random_key(std::mt19937_64 &rng, uint32_t K) {
    std::vector<uint8_t> c(K);
    for (auto &x : c) x = static_cast<uint8_t>(rng() & 3u);
    return key_of(c, K);
}

bool same(const JumpKey &a, const JumpKey &b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3]; }

int fail(const char *what, uint32_t K) {
    std::printf("FAIL: %s (K = %u)\n", what, K);
    return 1;
}

}  // namespace

int main() {
    std::mt19937_64 rng(2024);
    uint64_t checks = 0;
    const char acgt[] = "ACGT";
    for (uint32_t K : {16u, 17u, 31u, 44u, 52u, 60u, 63u, 64u}) {
        // key packing: the read's last K symbols in consumption order == the low 2K bits of its packed form (the staged LDS words)
        for (int rep = 0; rep < 200; ++rep) {
            const uint64_t m = K + rng() % 80;
            std::vector<uint8_t> q(m);
            for (auto &c : q) c = static_cast<uint8_t>(acgt[rng() & 3u]);
            std::vector<uint32_t> packed(((m + 63) / 64) * 4 + 4, 0);
            if (!rbg_hostpath::pack_read_acgt(q.data(), m, packed.data())) return fail("packer refused an ACGT read", K);
            JumpKey staged{{packed[0], packed[1], packed[2], packed[3]}};
            jump_key_mask(staged, K);
            std::vector<uint8_t> cons(K);
            for (uint32_t t = 0; t < K; ++t) cons[t] = static_cast<uint8_t>(q[m - 1 - t] == 'A' ? 0 : q[m - 1 - t] == 'C' ? 1 : q[m - 1 - t] == 'G' ? 2 : 3);
            if (!same(staged, key_of(cons, K))) return fail("staged words and the symbol-by-symbol key differ", K);
            // what lies beyond K does not reach the key
            JumpKey noisy = staged;
            for (uint32_t t = K; t < kJumpMaxK; ++t) jump_key_set(noisy, t, static_cast<uint32_t>(rng() & 3u));
            jump_key_mask(noisy, K);
            if (!same(noisy, staged)) return fail("bits beyond 2K survived the mask", K);
            ++checks;
        }
        // a full chain: seven keys with one home bucket fill it and the three after it; each is found where it went, an absent key
        // with the same home is refused at the first empty slot, not before
        {
            HostTable T(16);
            const uint64_t home = 5;
            std::vector<JumpKey> chain;
            while (chain.size() < 8) {
                const JumpKey k = random_key(rng, K);
                if (jump_home(jump_hash(k), T.nb) == home) chain.push_back(k);
            }
            for (uint32_t i = 0; i < 7; ++i)
                if (T.insert(chain[i], i, i + 10, i + 100) != home + i / 2) return fail("insert left the chain", K);
            for (uint32_t i = 0; i < 7; ++i) {
                uint32_t v[3], nbk = 0;
                if (!T.probe(chain[i], v, nbk) || v[0] != i || v[1] != i + 10 || v[2] != i + 100) return fail("chained key not found", K);
                if (nbk != i / 2 + 1) return fail("probe read the wrong number of buckets", K);
                ++checks;
            }
            uint32_t v[3], nbk = 0;
            if (T.probe(chain[7], v, nbk)) return fail("absent key found", K);
            if (nbk != 4) return fail("absent key's probe did not end at the first empty slot", K);
            ++checks;
        }
        // wrap-around: keys whose home is the last bucket continue at bucket 0
        {
            HostTable T(8);
            std::vector<JumpKey> ks;
            while (ks.size() < 5) {
                const JumpKey k = random_key(rng, K);
                if (jump_home(jump_hash(k), T.nb) == T.nb - 1) ks.push_back(k);
            }
            for (uint32_t i = 0; i < 4; ++i) T.insert(ks[i], 7 * i, 7 * i + 1, 0xFFFFFFFFu);
            for (uint32_t i = 0; i < 4; ++i) {
                uint32_t v[3], nbk = 0;
                if (!T.probe(ks[i], v, nbk) || v[0] != 7 * i || v[2] != 0xFFFFFFFFu) return fail("wrapped key not found", K);
                if (nbk != i / 2 + 1) return fail("wrapped probe read the wrong number of buckets", K);
                ++checks;
            }
            uint32_t v[3], nbk = 0;
            if (T.probe(ks[4], v, nbk) || nbk != 3) return fail("absent key of a wrapped chain", K);
            ++checks;
        }
        // keys that differ only in their last symbol (the read's first of the K)
        {
            HostTable T(64);
            std::vector<uint8_t> c(K);
            for (auto &x : c) x = static_cast<uint8_t>(rng() & 3u);
            const JumpKey a = key_of(c, K);
            c[K - 1] ^= 1u;
            const JumpKey b = key_of(c, K);
            c[K - 1] ^= 3u;
            const JumpKey d = key_of(c, K);
            T.insert(a, 1, 2, 3);
            uint32_t v[3], nbk = 0;
            if (T.probe(b, v, nbk)) return fail("a key one last symbol away was taken for another", K);
            T.insert(b, 4, 5, 6);
            if (!T.probe(a, v, nbk) || v[0] != 1) return fail("first of two near keys", K);
            if (!T.probe(b, v, nbk) || v[0] != 4) return fail("second of two near keys", K);
            if (T.probe(d, v, nbk)) return fail("third near key found without being inserted", K);
            checks += 4;
        }
    }
    // a table at the build's load (one key per bucket) with random keys: every key found, random absent keys refused, short chains
    {
        const uint64_t n = 100000;
        HostTable T(jump_buckets_for(n));
        std::vector<JumpKey> ks;
        for (uint64_t i = 0; i < n; ++i) ks.push_back(random_key(rng, 52));
        for (uint64_t i = 0; i < n; ++i) T.insert(ks[i], static_cast<uint32_t>(i), static_cast<uint32_t>(i), 0);
        uint64_t total = 0, worst = 0;
        for (uint64_t i = 0; i < n; ++i) {
            uint32_t v[3], nbk = 0;
            if (!T.probe(ks[i], v, nbk) || v[0] != i) return fail("key of the loaded table not found", 52);
            total += nbk;
            if (nbk > worst) worst = nbk;
        }
        if (total > n * 3 / 2) return fail("mean chain longer than 1.5 buckets at load one half", 52);
        ++checks;
        std::printf("load 0.5: %.3f buckets per hit, worst %llu\n", double(total) / n, static_cast<unsigned long long>(worst));
    }
    std::printf("jump table ok %llu\n", static_cast<unsigned long long>(checks));
    return 0;
}
