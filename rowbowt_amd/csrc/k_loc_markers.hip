// k_loc_markers.hip -- markers at located text positions: what rb_locs prints per read (the reference's rb_markers_tsa.cpp:76-88 -- for every location l of
// the read's longest greedy seed, the markers of the text-position table that overlap [l, l + m - 1]).  Input is what K3 leaves on the device (locs, loc_off)
// and the reads' offsets; output is ragged per READ: mk_off[N + 1] and the values, location after location, run order within a location.
//
// PARTITION.  A group of G lanes owns one read (G = 4, 16 or 64) and strides over its locations, one marker_query per lane and location: neighbouring
// locations of a read come off a phi chain and are unrelated text positions, so every query is its own sector whoever asks it, and the only thing to
// get right is that a read with 3 locations does not hold 64 lanes and a read with 3000 is not walked by one.  Nothing is kept per location: the count
// pass reduces over the group and writes one total per read, the fill pass repeats the queries in rounds of G locations and places a round's values by a
// group-wide exclusive prefix over the round's counts on top of a running base.  The scratch is the scan's, for N items.
// G is chosen ON THE DEVICE: the number of locations is loc_off[N], which the host does not have without a synchronisation that the _dev calls never make.
// One kernel holds the three widths and branches on a value every lane agrees on; RBG_LOCMK_GROUP (4 / 16 / 64) forces one for tests and A/Bs.
#include "rbg_device.hpp"

namespace rbg {
namespace {

// the group width for an average of L / N locations per read: the width that idles the fewest lanes at 3, 30 and 300 locations per read
// (tools/loc_markers_rate.py times all three beside it)
__device__ __forceinline__ int loc_group_for(const uint64_t L, const uint64_t N) {
    if (L <= 8 * N) return 4;
    if (L <= 96 * N) return 16;
    return 64;
}

template <int G>
__device__ __forceinline__ unsigned long long group_sum(unsigned long long v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
    return v;
}
// inclusive prefix over the G lanes of a group (g = lane within the group)
template <int G>
__device__ __forceinline__ unsigned long long group_scan(unsigned long long v, const int g) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
        const unsigned long long u = __shfl_up(v, o, G);
        if (g >= o) v += u;
    }
    return v;
}

// one location of a read of length m against the text table, in wrapping 64-bit arithmetic: [l, l + m - 1]; empty when the end lies below the start
// (m == 0, or a location that wrapped below zero whose end wraps back), marker_query drops lo >= n (a wrapped location that does not wrap back) and
// clamps hi to n - 1 (a read overhanging the end of the text) -- so the bucket index stays inside the directory
__device__ __forceinline__ uint64_t loc_query(const MkView &v, const uint64_t l, const uint64_t m, uint64_t *src) {
    const uint64_t hi = l + m - 1;
    uint64_t c;
    if (hi < l || !marker_query(v, l, hi, src, &c)) return 0;
    return c;
}

template <int G>
__device__ __forceinline__ void loc_markers_count(const MkView &v, const uint64_t *__restrict__ locs, const uint64_t *__restrict__ loc_off,
                                                  const uint64_t *__restrict__ off, const uint64_t N, uint64_t *__restrict__ out) {
    const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t groups = static_cast<uint64_t>(gridDim.x) * blockDim.x / G;
    const int g = static_cast<int>(threadIdx.x) & (G - 1);
    for (uint64_t i = tid / G; i < N; i += groups) {
        const uint64_t m = off[i + 1] - off[i], e = loc_off[i + 1];
        unsigned long long total = 0;
        for (uint64_t j = loc_off[i] + g; j < e; j += G) {
            uint64_t src;
            total += loc_query(v, locs[j], m, &src);
        }
        total = group_sum<G>(total);
        if (g == 0) out[i + 1] = total;
    }
}

template <int G>
__device__ __forceinline__ void loc_markers_fill(const MkView &v, const uint64_t *__restrict__ locs, const uint64_t *__restrict__ loc_off,
                                                 const uint64_t *__restrict__ off, const uint64_t N, const uint64_t *__restrict__ mk_off,
                                                 uint64_t *__restrict__ mk) {
    const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t groups = static_cast<uint64_t>(gridDim.x) * blockDim.x / G;
    const int g = static_cast<int>(threadIdx.x) & (G - 1);
    const RBG_GLOBAL uint64_t *vals = as_global(v.vals);
    for (uint64_t i = tid / G; i < N; i += groups) {
        uint64_t base = mk_off[i];
        if (mk_off[i + 1] == base) continue;   // (the same for every lane of the group)
        const uint64_t m = off[i + 1] - off[i], e = loc_off[i + 1];
        for (uint64_t j0 = loc_off[i]; j0 < e; j0 += G) {   // a round: G locations, the group's lanes side by side
            const uint64_t j = j0 + g;
            uint64_t src = 0;
            const unsigned long long c = j < e ? loc_query(v, locs[j], m, &src) : 0ull;
            const unsigned long long incl = group_scan<G>(c, g);
            uint64_t *dst = mk + base + (incl - c);
            for (uint64_t t = 0; t < c; ++t) dst[t] = vals[src + t];
            base += __shfl(incl, G - 1, G);
        }
    }
}

// LAUNCH BOUNDS: 256 threads, eight waves per SIMD.  The three widths together take 56 VGPRs in the count kernel; the fill kernel took 65 left to
// itself and takes 64 when asked for the eight waves, without scratch (tools/kernel_resources.py)
__global__ __launch_bounds__(256) void k_loc_markers_count(const DevIndex ix, const uint64_t *__restrict__ locs, const uint64_t *__restrict__ loc_off,
                                                           const uint64_t *__restrict__ off, const uint64_t N, uint64_t *__restrict__ out, const int group) {
    const MkView v = text_marker_view(ix);
    const int G = group ? group : loc_group_for(loc_off[N], N);
    if (G == 4) loc_markers_count<4>(v, locs, loc_off, off, N, out);
    else if (G == 16) loc_markers_count<16>(v, locs, loc_off, off, N, out);
    else loc_markers_count<64>(v, locs, loc_off, off, N, out);
    if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = 0;
}

__global__ __launch_bounds__(256, 8) void k_loc_markers_fill(const DevIndex ix, const uint64_t *__restrict__ locs, const uint64_t *__restrict__ loc_off,
                                                          const uint64_t *__restrict__ off, const uint64_t N, const uint64_t *__restrict__ mk_off,
                                                          uint64_t *__restrict__ mk, const int group) {
    const MkView v = text_marker_view(ix);
    const int G = group ? group : loc_group_for(loc_off[N], N);
    if (G == 4) loc_markers_fill<4>(v, locs, loc_off, off, N, mk_off, mk);
    else if (G == 16) loc_markers_fill<16>(v, locs, loc_off, off, N, mk_off, mk);
    else loc_markers_fill<64>(v, locs, loc_off, off, N, mk_off, mk);
}

// the grid for the widest group: a narrower one finds more groups in the same threads (the loops stride by the groups there are)
inline int loc_grid(const LaunchCfg &cfg, const uint64_t N, const int group) {
    const uint64_t w = group ? static_cast<uint64_t>(group) : 64u;
    return grid_for(cfg, N > (~uint64_t(0)) / w ? ~uint64_t(0) : N * w);
}

}  // namespace

int loc_markers_group() {
    const char *e = std::getenv("RBG_LOCMK_GROUP");
    if (!e || !*e) return 0;
    const int g = std::atoi(e);
    return g == 4 || g == 16 || g == 64 ? g : 0;
}

int launch_loc_markers_plan(const DevIndex &ix, const LaunchCfg &cfg, const uint64_t *locs, const uint64_t *loc_off, const uint64_t *off, uint64_t N,
                            uint64_t *mk_off, void *tmp, size_t tmp_bytes, int group, void *stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (N == 0) return static_cast<int>(hipMemsetAsync(mk_off, 0, 8, st));
    hipLaunchKernelGGL(k_loc_markers_count, dim3(loc_grid(cfg, N, group)), dim3(cfg.block_threads), 0, st, ix, locs, loc_off, off, N, mk_off, group);
    int rc = static_cast<int>(hipGetLastError());
    if (rc) return rc;
    return scan_in_place(mk_off + 1, N, tmp, tmp_bytes, st);
}

int launch_loc_markers_fill(const DevIndex &ix, const LaunchCfg &cfg, const uint64_t *locs, const uint64_t *loc_off, const uint64_t *off, uint64_t N,
                            const uint64_t *mk_off, uint64_t *mk, int group, void *stream) {
    if (N == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_loc_markers_fill, dim3(loc_grid(cfg, N, group)), dim3(cfg.block_threads), 0, st, ix, locs, loc_off, off, N, mk_off, mk, group);
    return static_cast<int>(hipGetLastError());
}

}  // namespace rbg
