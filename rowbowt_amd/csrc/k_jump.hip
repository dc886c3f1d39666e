// k_jump.hip -- load-time construction of the jump table (rbg_jump.h): the state after every K-mer that occurs in the text.
// The K-mers that occur are enumerated by backward extension, one symbol per level: level l holds every l-symbol word that occurs
// (its SA interval is non-empty) with that interval; each is extended by the four major symbols with the one-symbol LF of the
// layout (launch_lf: RowBowt::LF, rowbowt.hpp:74-88) and the non-empty children are appended to the next level.  The final level's
// words are then searched as packed reads by k_find_range_runs itself -- so the table holds exactly the {lo, hi, toehold} the
// search computes (the toehold arithmetic and re-samples of rowbowt.hpp:555-573 included) -- and inserted with atomics.
#include "rbg_device.hpp"
#include "rbg_jump.h"

namespace rbg {
namespace {

// children of the parents [base, base + cnt): child j = (parent base + j / 4, major index j % 4)
__global__ __launch_bounds__(256) void k_jump_expand(const uint64_t *__restrict__ plo, const uint64_t *__restrict__ phi, const uint64_t base,
                                                     const uint64_t cnt, const uint8_t *__restrict__ major_byte, uint64_t *__restrict__ clo,
                                                     uint64_t *__restrict__ chi, uint8_t *__restrict__ sym) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < 4 * cnt; j += stride) {
        const uint64_t par = base + (j >> 2);
        clo[j] = plo[par];
        chi[j] = phi[par];
        sym[j] = major_byte[j & 3u];
    }
}

// the children that occur go to the next level: {lo, hi, parent key + symbol `level`} appended at *count (one atomic per wave)
__global__ __launch_bounds__(256) void k_jump_keep(const uint64_t *__restrict__ nlo, const uint64_t *__restrict__ nhi, const uint4 *__restrict__ pkey,
                                                   const uint64_t base, const uint64_t N, const uint32_t level, uint64_t *__restrict__ olo,
                                                   uint64_t *__restrict__ ohi, uint4 *__restrict__ okey, unsigned long long *__restrict__ count) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t wb = static_cast<uint64_t>(blockIdx.x) * blockDim.x + (threadIdx.x & ~(kWave - 1)); wb < N; wb += stride) {   // (whole waves)
        const uint64_t j = wb + lane;
        const bool keep = j < N && nlo[j] <= nhi[j];
        const uint64_t bal = __ballot(keep);
        unsigned long long at = 0;
        if (lane == 0 && bal) at = atomicAdd(count, static_cast<unsigned long long>(__popcll(bal)));
        at = __shfl(at, 0);
        if (keep) {
            const uint64_t o = at + static_cast<uint64_t>(__popcll(bal & ((uint64_t(1) << lane) - 1u)));
            uint4 kk = pkey[base + (j >> 2)];
            JumpKey key{{kk.x, kk.y, kk.z, kk.w}};
            jump_key_set(key, level, static_cast<uint32_t>(j & 3u));
            olo[o] = nlo[j];
            ohi[o] = nhi[j];
            okey[o] = make_uint4(key.w[0], key.w[1], key.w[2], key.w[3]);
        }
    }
}

// the final level's words as packed reads of K symbols: one 16-byte chunk each
__global__ __launch_bounds__(256) void k_jump_meta(const uint64_t cnt, const uint32_t K, uint2 *__restrict__ meta) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < cnt; i += stride)
        meta[i] = make_uint2(static_cast<uint32_t>(i), K);
}

// insert the searched words: claim a slot by its tag, then write key and state
__global__ __launch_bounds__(256) void k_jump_insert(const uint4 *__restrict__ keys, const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi,
                                                     const uint64_t *__restrict__ ss, const uint64_t cnt, uint32_t *__restrict__ tab, const uint64_t nb,
                                                     unsigned long long *__restrict__ inserted) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < cnt; i += stride) {
        const uint64_t l = lo[i], h = hi[i], k = ss ? ss[i] : 0;
        if (l > h || h > 0xFFFFFFFFull) continue;
        uint32_t kk;
        if (k == ~uint64_t(0)) kk = 0xFFFFFFFFu;                  // (as ftab_lookup: the word's last row is text position 0)
        else if (k >= 0xFFFFFFF0ull) continue;                     // not expressible: the read takes the ftab path
        else kk = static_cast<uint32_t>(k);
        const uint4 kw = keys[i];
        const JumpKey key{{kw.x, kw.y, kw.z, kw.w}};
        uint64_t b = jump_home(jump_hash(key), nb);
        for (uint64_t step = 0; step < nb; ++step) {
            bool done = false;
            for (uint32_t s = 0; s < 2 && !done; ++s) {
                uint32_t *slot = tab + (2 * b + s) * kJumpSlotWords;
                if (atomicCAS(slot + 7, kJumpEmptyTag, kJumpFullTag) == kJumpEmptyTag) {
                    reinterpret_cast<uint4 *>(slot)[0] = kw;
                    reinterpret_cast<uint4 *>(slot)[1] = make_uint4(static_cast<uint32_t>(l), static_cast<uint32_t>(h), kk, kJumpFullTag);
                    done = true;
                }
            }
            if (done) { atomicAdd(inserted, 1ull); break; }
            b = b + 1 == nb ? 0 : b + 1;
        }
    }
}

struct DevBuf {   // scratch of the build: freed on every path out
    void *p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t b) { bytes = b; return hipMalloc(&p, b ? b : 1); }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

}  // namespace

// children per pass (parents x 4): bounds the scratch of a level whatever the frontier
constexpr uint64_t kJumpChunkParents = uint64_t(1) << 24;

int launch_build_jump(const DevIndex &ix, const LaunchCfg &cfg, uint32_t K, uint64_t table_budget, uint64_t peak_budget, void **tab,
                      uint64_t *tab_bytes, uint64_t *buckets, uint64_t *keys, const char **why, void *stream) {
    *tab = nullptr; *tab_bytes = 0; *buckets = 0; *keys = 0; *why = nullptr;
    if (ix.pos_bytes != 4) { *why = "8-byte positions (the table holds 4-byte states)"; return 0; }
    if (ix.layout != 2 || ix.nmajor != 4 || !ix.stage_ok) { *why = "only the staged search of the run-indexed layout over four major symbols uses it"; return 0; }
    if (K < kJumpMinK || K > kJumpMaxK) return static_cast<int>(hipErrorInvalidValue);
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevIndex plain = ix;   // the words are searched WITHOUT a jump table
    plain.jump = nullptr;
    plain.jump_buckets = 0;
    plain.jump_k = 0;
    // scratch: two levels of {lo, hi, key} (32 bytes a word) and one pass of children (4 C x 33 bytes); the pass takes at most a quarter
    // of `peak_budget`, and every allocation is checked against it BEFORE it is made (scratch + table never exceed it)
    uint64_t C = kJumpChunkParents;
    while (C > (uint64_t(1) << 12) && 4 * C * 33 > peak_budget / 4) C >>= 1;
    if (4 * C * 33 + 1024 > peak_budget) { *why = "its build scratch exceeds what the HBM budget leaves"; return 0; }
    DevBuf clo, chi, nlo, nhi, sym, mb, cnt_d;
    DevBuf lv_lo[2], lv_hi[2], lv_key[2];
    uint64_t cap[2] = {0, 0};
    hipError_t e = hipSuccess;
    auto scratch = [&]() {
        return clo.bytes + chi.bytes + nlo.bytes + nhi.bytes + sym.bytes + 32 * (cap[0] + cap[1]);
    };
    bool over = false;   // set by grow: the larger level would not fit peak_budget (nothing allocated)
    auto grow = [&](int w, uint64_t need, uint64_t used) -> hipError_t {   // level w holds `used` words; make room for `need`
        if (need <= cap[w]) return hipSuccess;
        const uint64_t nc = std::max<uint64_t>(need, cap[w] + cap[w] / 2);
        if (scratch() + 32 * nc > peak_budget) { over = true; return hipSuccess; }   // (old and new level side by side while copying)
        DevBuf a, b, c;
        hipError_t r = a.alloc(nc * 8);
        if (r == hipSuccess) r = b.alloc(nc * 8);
        if (r == hipSuccess) r = c.alloc(nc * 16);
        if (r == hipSuccess && used) r = hipMemcpyAsync(a.p, lv_lo[w].p, used * 8, hipMemcpyDeviceToDevice, st);
        if (r == hipSuccess && used) r = hipMemcpyAsync(b.p, lv_hi[w].p, used * 8, hipMemcpyDeviceToDevice, st);
        if (r == hipSuccess && used) r = hipMemcpyAsync(c.p, lv_key[w].p, used * 16, hipMemcpyDeviceToDevice, st);
        if (r == hipSuccess) r = hipStreamSynchronize(st);
        if (r != hipSuccess) return r;
        std::swap(lv_lo[w].p, a.p); std::swap(lv_lo[w].bytes, a.bytes);
        std::swap(lv_hi[w].p, b.p); std::swap(lv_hi[w].bytes, b.bytes);
        std::swap(lv_key[w].p, c.p); std::swap(lv_key[w].bytes, c.bytes);
        cap[w] = nc;
        return hipSuccess;
    };
    e = clo.alloc(4 * C * 8);
    if (e == hipSuccess) e = chi.alloc(4 * C * 8);
    if (e == hipSuccess) e = nlo.alloc(4 * C * 8);
    if (e == hipSuccess) e = nhi.alloc(4 * C * 8);
    if (e == hipSuccess) e = sym.alloc(4 * C);
    if (e == hipSuccess) e = mb.alloc(256);
    if (e == hipSuccess) e = cnt_d.alloc(2 * sizeof(unsigned long long));
    if (e == hipSuccess) {   // major index -> byte (launch_build_ftab does the same)
        uint8_t lut2[256], inv[256] = {0};
        e = hipMemcpy(lut2, ix.lut2, 256, hipMemcpyDeviceToHost);
        for (int b = 0; b < 256; ++b)
            if (lut2[b] != 0xFF) inv[lut2[b] & 3u] = static_cast<uint8_t>(b);
        if (e == hipSuccess) e = hipMemcpy(mb.p, inv, 256, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = grow(0, 1, 0);
    if (e == hipSuccess && over) { *why = "its build scratch exceeds what the HBM budget leaves"; return 0; }
    if (e == hipSuccess) {   // level 0: the empty word, full_range() (rowbowt.hpp:115-118)
        const uint64_t lo0 = 0, hi0 = ix.n - 1;
        const uint4 k0 = make_uint4(0, 0, 0, 0);
        e = hipMemcpy(lv_lo[0].p, &lo0, 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(lv_hi[0].p, &hi0, 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(lv_key[0].p, &k0, 16, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) return static_cast<int>(e);
    uint64_t F = 1;
    int cur = 0;
    for (uint32_t level = 0; level < K; ++level) {
        const int nx = cur ^ 1;
        const unsigned long long zero = 0;
        if ((e = hipMemcpy(cnt_d.p, &zero, sizeof(zero), hipMemcpyHostToDevice)) != hipSuccess) return static_cast<int>(e);
        uint64_t used = 0;
        for (uint64_t base = 0; base < F; base += C) {
            const uint64_t cnt = std::min<uint64_t>(C, F - base);
            if ((e = grow(nx, used + 4 * cnt, used)) != hipSuccess) return static_cast<int>(e);
            if (over) { *why = "its build scratch exceeds what the HBM budget leaves"; return 0; }
            hipLaunchKernelGGL(k_jump_expand, dim3(grid_for(cfg, 4 * cnt)), dim3(256), 0, st, lv_lo[cur].as<uint64_t>(), lv_hi[cur].as<uint64_t>(), base, cnt,
                               mb.as<uint8_t>(), clo.as<uint64_t>(), chi.as<uint64_t>(), sym.as<uint8_t>());
            if ((e = hipGetLastError()) != hipSuccess) return static_cast<int>(e);
            if (int rc = launch_lf(plain, cfg, clo.as<uint64_t>(), chi.as<uint64_t>(), sym.as<uint8_t>(), 4 * cnt, nlo.as<uint64_t>(), nhi.as<uint64_t>(), st)) return rc;
            hipLaunchKernelGGL(k_jump_keep, dim3(grid_for(cfg, 4 * cnt)), dim3(256), 0, st, nlo.as<uint64_t>(), nhi.as<uint64_t>(), lv_key[cur].as<uint4>(), base,
                               4 * cnt, level, lv_lo[nx].as<uint64_t>(), lv_hi[nx].as<uint64_t>(), lv_key[nx].as<uint4>(), cnt_d.as<unsigned long long>());
            if ((e = hipGetLastError()) != hipSuccess) return static_cast<int>(e);
            unsigned long long got = 0;
            if ((e = hipMemcpyAsync(&got, cnt_d.p, sizeof(got), hipMemcpyDeviceToHost, st)) != hipSuccess) return static_cast<int>(e);
            if ((e = hipStreamSynchronize(st)) != hipSuccess) return static_cast<int>(e);
            used = got;
        }
        F = used;
        cur = nx;
        if (F == 0) break;
    }
    *keys = F;
    const uint64_t nb = jump_buckets_for(F);
    const uint64_t bytes = nb * kJumpBucketBytes;
    if (F == 0 || nb >= (uint64_t(1) << 32)) { *why = F ? "more keys than the table addresses" : "no K-mer occurs"; return 0; }
    if (bytes > table_budget || bytes + scratch() > peak_budget) {
        *why = "the table exceeds the bytes allowed for it (what the HBM budget leaves; by default also half the replica)";
        return 0;
    }
    void *t = nullptr;
    if ((e = hipMalloc(&t, bytes)) != hipSuccess) { (void)hipGetLastError(); *why = "hipMalloc of the table failed"; return 0; }
    int rc = static_cast<int>(hipMemsetAsync(t, 0, bytes, st));
    if (!rc) rc = static_cast<int>(hipMemsetAsync(cnt_d.p, 0, sizeof(unsigned long long), st));
    // the final level, searched as packed reads (one 16-byte chunk each) by the search kernel itself; chunks of 4 C words in the
    // children's scratch: meta in clo, lo / hi / toehold in chi / nlo / nhi
    for (uint64_t base = 0; !rc && base < F; base += 4 * C) {
        const uint64_t cnt = std::min<uint64_t>(4 * C, F - base);
        hipLaunchKernelGGL(k_jump_meta, dim3(grid_for(cfg, cnt)), dim3(256), 0, st, cnt, K, clo.as<uint2>());
        rc = static_cast<int>(hipGetLastError());
        if (!rc) rc = launch_find_range_runs_packed(plain, cfg, clo.as<uint2>(), lv_key[cur].as<uint4>() + base, cnt, chi.as<uint64_t>(), nlo.as<uint64_t>(),
                                                    ix.has_tsa ? nhi.as<uint64_t>() : nullptr, st);
        if (!rc) {
            hipLaunchKernelGGL(k_jump_insert, dim3(grid_for(cfg, cnt)), dim3(256), 0, st, lv_key[cur].as<uint4>() + base, chi.as<uint64_t>(), nlo.as<uint64_t>(),
                               ix.has_tsa ? nhi.as<uint64_t>() : nullptr, cnt, static_cast<uint32_t *>(t), nb, cnt_d.as<unsigned long long>());
            rc = static_cast<int>(hipGetLastError());
        }
    }
    unsigned long long ins = 0;
    if (!rc) rc = static_cast<int>(hipMemcpyAsync(&ins, cnt_d.p, sizeof(ins), hipMemcpyDeviceToHost, st));
    if (!rc) rc = static_cast<int>(hipStreamSynchronize(st));
    if (rc) { (void)hipFree(t); return rc; }
    *tab = t;
    *tab_bytes = bytes;
    *buckets = nb;
    *keys = ins;
    return 0;
}

}  // namespace rbg
