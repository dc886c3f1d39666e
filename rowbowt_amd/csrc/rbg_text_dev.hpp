// rbg_text_dev.hpp -- decimals written by kernels: what k_text.hip (rbg_align_text) and k_report.hip (rbg_markers_report_text) share.
#ifndef RBG_TEXT_DEV_HPP
#define RBG_TEXT_DEV_HPP
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RBG_TEXT_D __device__ __forceinline__
#else
#define RBG_TEXT_D inline   // a host compiler: tests/cpp/text_dec_check.cpp checks these against snprintf
#endif

#include <cstdint>

namespace rbg {

RBG_TEXT_D uint32_t dec_len(uint64_t v) {
    uint32_t n = 1;
    if (v >= 10000000000000000ull) { v /= 10000000000000000ull; n += 16; }
    if (v >= 100000000ull) { v /= 100000000ull; n += 8; }
    if (v >= 10000ull) { v /= 10000ull; n += 4; }
    if (v >= 100ull) { v /= 100ull; n += 2; }
    if (v >= 10ull) n += 1;
    return n;
}
// the n = dec_len(v) digits of v at p[0 .. n)
template <typename Ptr>
RBG_TEXT_D void put_dec(Ptr p, uint64_t v, uint32_t n) {
    for (uint32_t j = n; j-- > 0;) {
        const uint64_t q = v / 10;
        p[j] = static_cast<char>('0' + static_cast<uint32_t>(v - q * 10));
        v = q;
    }
}

}  // namespace rbg
#endif
