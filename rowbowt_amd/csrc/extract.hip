// extract.hip -- the indexed text read back from the index: the row of a text position (rbg_isa_dev) and the bases of text intervals (rbg_extract_dev),
// over the ISA sample of rbg_isa.hpp and the FL index of rbg_fl.hpp (include/rbg.h; rbg_extract_prepare builds and uploads both).  Templated on the
// position width only: neither structure depends on the rank layout.
//
//   k_isa_rows   one lane per position, grid-stride: the sample before p (directory pair, bounded bisection), then p - q FL steps from its row; row[j] =
//                the row of the suffix at p.  A position >= n gives row 0 and sets the error word.
//   k_extract    one lane per item {pos, len, out_off}, grid-stride: the same lookup and walk-in, then up to len FL steps, each giving the current row's F
//                byte; the walk ends at the first row without a base (terminator, separator, N, anything else) and got[j] = the bases produced.  Exactly
//                len bytes are written at out + out_off: the bases, then zeros.  The bases are gathered four to a register and leave as aligned 32-bit
//                words; single bytes are stored only where the item's first and last word are partial.  A position >= n writes len zeros, got 0, and
//                sets the error word.
//
// An FL chain is serial: the parallelism of a long interval comes from splitting it into items, each of which finds its own row through the samples
// (rbg_extract does that on the host before the upload).  The walk's state stays in registers: no scratch.  FlView and IsaView are staged in LDS as in
// k_extend_right: a lane picks its base's lists by an index, and indexing kernel arguments by a lane value would put them in scratch.
#include "rbg_isa.hpp"
#include "rbg_launch.hpp"
#include "rbg_sam_dev.hpp"

namespace rbg {
namespace {

template <typename P>
__global__ __launch_bounds__(256) void k_isa_rows(const FlView fl, const IsaView isa, const uint64_t *__restrict__ pos, const uint64_t M,
                                                  uint64_t *__restrict__ row, unsigned int *__restrict__ err) {
    __shared__ FlView s_fl;
    __shared__ IsaView s_isa;
    if (threadIdx.x == 0) { s_fl = fl; s_isa = isa; }
    __syncthreads();
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < M; i += stride) {
        const uint64_t p = pos[i];
        if (p >= s_isa.n) {
            row[i] = 0;
            atomicOr(err, 1u);
            continue;
        }
        const uint64_t r = isa_row<P>(s_isa, s_fl, p);
        if (r == kFlNone) atomicOr(err, 2u);      // (a row without a base on a walk-in: the samples are not a BWT's)
        row[i] = r == kFlNone ? 0 : r;
    }
}

// the bytes of one item on their way out: up to four in `w`, the lowest at dst[at - held .. at)
struct WordOut {
    uint8_t *dst;
    uint32_t w, held;
    __device__ __forceinline__ void put(const uint64_t at, const uint32_t c, const bool last) {
        const uint32_t lane = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(dst + at) & 3u);
        w |= c << (8 * lane);
        held += 1;
        if (lane != 3 && !last) return;
        if (held == 4) {
            *reinterpret_cast<uint32_t *>(dst + at - 3) = w;      // (held == 4 ends at lane 3: the address is aligned)
        } else {
            for (uint32_t k = 0; k < held; ++k) dst[at - k] = static_cast<uint8_t>(w >> (8 * (lane - k)));
        }
        w = 0;
        held = 0;
    }
};

template <typename P>
__global__ __launch_bounds__(256) void k_extract(const FlView fl, const IsaView isa, const uint64_t *__restrict__ pos, const uint32_t *__restrict__ len,
                                                 const uint64_t *__restrict__ out_off, const uint64_t M, uint8_t *__restrict__ out, uint32_t *__restrict__ got,
                                                 unsigned int *__restrict__ err) {
    __shared__ FlView s_fl;
    __shared__ IsaView s_isa;
    if (threadIdx.x == 0) { s_fl = fl; s_isa = isa; }
    __syncthreads();
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < M; i += stride) {
        const uint64_t p = pos[i];
        const uint32_t L = len[i];
        uint64_t r = kFlNone;
        if (p >= s_isa.n) {
            atomicOr(err, 1u);
        } else if (L) {
            r = isa_row<P>(s_isa, s_fl, p);
            if (r == kFlNone) atomicOr(err, 2u);
        }
        WordOut o{out + out_off[i], 0u, 0u};
        uint32_t g = 0;
        bool live = r != kFlNone;
        for (uint32_t t = 0; t < L; ++t) {
            uint32_t c = 0;
            if (live) {
                const FlStep st = fl_step<P>(s_fl, r);      // the base at this row, and the row one base further right
                c = st.sym;
                r = st.next;
                live = c != 0;
                g += live ? 1u : 0u;
            }
            o.put(t, c, t + 1 == L);
        }
        got[i] = g;
    }
}

}  // namespace

int launch_isa_rows(const FlView &fl, const IsaView &isa, uint32_t pos_bytes, const uint64_t *pos, uint64_t M, uint64_t *row, unsigned int *d_err, uint32_t cap,
                    void *stream) {
    if (M == 0) return 0;
    const dim3 grid(sam_grid(M, 256, cap)), block(256);
    return with_pos(pos_bytes, [&](auto p) { return launch_grid(k_isa_rows<pos_t<decltype(p)>>, grid, block, 0, stream, fl, isa, pos, M, row, d_err); });
}

int launch_extract(const FlView &fl, const IsaView &isa, uint32_t pos_bytes, const uint64_t *pos, const uint32_t *len, const uint64_t *out_off, uint64_t M,
                   uint8_t *out, uint32_t *got, unsigned int *d_err, uint32_t cap, void *stream) {
    if (M == 0) return 0;
    const dim3 grid(sam_grid(M, 256, cap)), block(256);
    return with_pos(pos_bytes, [&](auto p) {
        return launch_grid(k_extract<pos_t<decltype(p)>>, grid, block, 0, stream, fl, isa, pos, len, out_off, M, out, got, d_err);
    });
}

}  // namespace rbg
