// rbg_launch.hpp -- the tail every launcher ends in, once per launch style: the stream cast, the launch geometry or LDS limit taken from the
// chosen kernel's pointer, hipLaunchKernelGGL, and the launch's error as the launcher's return value.  The kernel itself is chosen with
// rbg_dispatch.hpp's with_pos / with_flag.  Everything lives in an anonymous namespace: each unit gets its own inlined copy.
#pragma once

#include "rbg_device.hpp"
#include "rbg_dispatch.hpp"

namespace rbg {
namespace {

// plain grid: the launcher worked the geometry out itself
template <typename Kernel, typename... Args>
int launch_grid(Kernel kern, const dim3 grid, const dim3 block, const size_t lds, void *stream, const Args &...args) {
    hipLaunchKernelGGL(kern, grid, block, lds, static_cast<hipStream_t>(stream), args...);
    return static_cast<int>(hipGetLastError());
}

// the kernels that stage the k-mer records in dynamic LDS (rbg_device.hpp kmer_launch)
template <typename Kernel, typename... Args>
int launch_kmer(Kernel kern, const DevIndex &ix, const LaunchCfg &cfg, const uint64_t N, const int grid_cap, const uint32_t max_k, void *stream,
                const Args &...args) {
    const KmerLaunch L = kmer_launch(ix, cfg, N, kern, grid_cap, max_k);
    return launch_grid(kern, L.grid, L.block, L.lds, stream, args...);
}

// a kernel whose dynamic LDS (plus `static_lds` bytes of __shared__ arrays) may pass what it gets without asking (rbg_device.hpp raise_lds)
template <typename Kernel, typename... Args>
int launch_lds(Kernel kern, const dim3 grid, const dim3 block, const size_t lds, const size_t static_lds, void *stream, const Args &...args) {
    raise_lds(kern, lds, static_lds);
    return launch_grid(kern, grid, block, lds, stream, args...);
}

// The search and seeding kernels of the run-indexed layout run in 512-thread workgroups: the staged tables and the top level are shared by
// eight waves.  Half as many workgroups as the configuration asks of 256-thread ones.
inline LaunchCfg runs512_cfg(const LaunchCfg &cfg) {
    LaunchCfg c = cfg;
    c.block_threads = 512;
    c.max_blocks = cfg.max_blocks > 0 ? std::max(1, cfg.max_blocks / 2) : 256 * 16;
    return c;
}

}  // namespace
}  // namespace rbg
