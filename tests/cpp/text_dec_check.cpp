// CPU test of the decimals that the text kernels write (rowbowt_amd/csrc/rbg_text_dev.hpp: dec_len, put_dec) against snprintf("%llu"):
// 0, every 10^k - 1 / 10^k / 10^k + 1 for k = 1..19, every 2^k - 1 / 2^k for k = 1..63, 2^64 - 1, and 100 000 values of a fixed-seed generator
// spread evenly over the bit widths 1..64 (so every digit count 1..20 occurs hundreds of times at the least).  put_dec writes into the middle
// of a buffer whose bytes before and after the digits are sentinels, all of them checked after every call.  The first mismatch ends the run.
// Prints "text dec ok <checks>".
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../rowbowt_amd/csrc/rbg_text_dev.hpp"

namespace {

constexpr int kGuard = 32, kRoom = 24;
constexpr unsigned char kSentinel = 0xA5;
uint64_t g_checks = 0;

bool check(uint64_t v) {
    char want[32];
    const int wn = std::snprintf(want, sizeof want, "%llu", static_cast<unsigned long long>(v));
    const uint32_t n = rbg::dec_len(v);
    if (wn < 1 || n != static_cast<uint32_t>(wn)) {
        std::fprintf(stderr, "dec_len(%llu) = %u, snprintf wrote %d\n", static_cast<unsigned long long>(v), n, wn);
        return false;
    }
    std::vector<unsigned char> buf(kGuard + kRoom + kGuard, kSentinel);   // (on the heap: ASan sees a write past either end as well)
    rbg::put_dec(reinterpret_cast<char *>(buf.data()) + kGuard, v, n);
    if (std::memcmp(buf.data() + kGuard, want, n) != 0) {
        std::fprintf(stderr, "put_dec(%llu): got %.*s, want %s\n", static_cast<unsigned long long>(v), static_cast<int>(n), reinterpret_cast<char *>(buf.data()) + kGuard, want);
        return false;
    }
    for (int j = 0; j < kGuard + kRoom + kGuard; ++j)
        if ((j < kGuard || j >= kGuard + static_cast<int>(n)) && buf[j] != kSentinel) {
            std::fprintf(stderr, "put_dec(%llu): byte %d outside its %u digits was written\n", static_cast<unsigned long long>(v), j - kGuard, n);
            return false;
        }
    ++g_checks;
    return true;
}

}  // namespace

int main() {
    bool ok = check(0);
    uint64_t p10 = 1;
    for (int k = 1; k <= 19; ++k) {
        p10 *= 10;
        ok = ok && check(p10 - 1) && check(p10) && check(p10 + 1);
    }
    for (int k = 1; k <= 63; ++k) {
        const uint64_t p2 = uint64_t(1) << k;
        ok = ok && check(p2 - 1) && check(p2);
    }
    ok = ok && check(~uint64_t(0));
    std::mt19937_64 rng(20240607);
    int widths[21] = {0};
    for (int t = 0; t < 100000 && ok; ++t) {
        const int bits = 1 + t % 64;                                        // every width alike often
        const uint64_t v = bits == 64 ? rng() : rng() & ((uint64_t(1) << bits) - 1);
        widths[rbg::dec_len(v) <= 20 ? rbg::dec_len(v) : 0] += 1;
        ok = check(v);
    }
    for (int d = 1; d <= 20 && ok; ++d)
        if (widths[d] < 100) { std::fprintf(stderr, "only %d random values of %d digits\n", widths[d], d); ok = false; }
    if (!ok) return 1;
    std::printf("text dec ok %" PRIu64 "\n", g_checks);
    return 0;
}
