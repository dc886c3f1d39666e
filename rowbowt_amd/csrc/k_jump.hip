// k_jump.hip -- load-time construction of the jump table (rbg_jump.h): the state after every K-mer that occurs in the text.
// The K-mers that occur are enumerated by backward extension, one symbol per level: level l holds every l-symbol word that occurs
// (its SA interval is non-empty) with that interval; each is extended by the four major symbols with the one-symbol LF of the
// layout (launch_lf: RowBowt::LF, rowbowt.hpp:74-88) and the non-empty children are appended to the next level.  The final level's
// words are then searched as packed reads by k_find_range_runs itself -- so the table holds exactly the {lo, hi, toehold} the
// search computes (the toehold arithmetic and re-samples of rowbowt.hpp:555-573 included) -- and inserted with atomics.
//
// Level 2 (rbg_jump.h): the extension goes on from the K-mers for K2 more symbols and the words of K + K2 symbols are searched and
// inserted into a second table the same way.  A build with a level 2 keeps WIDE records of a word: 32 bytes, the word's symbols in
// consumption order as two packed chunks (words 0..6: at most 112 symbols) and, in word 7, lo of the word's first K symbols -- the
// K-mer's name in the key of level 2.  The kernels are the same ones; the width and the two K travel in the high bits of the scalar
// arguments they have (kJumpWide, kJumpStamp, jump_insert_nb below), so that a build without level 2 runs exactly what it ran before.
#include <chrono>

#include "rbg_device.hpp"
#include "rbg_jump.h"

namespace rbg {
namespace {

constexpr uint32_t kJumpWide = 0x80000000u;    // k_jump_keep `level`, k_jump_meta `K`: the records are wide (two uint4 a word)
constexpr uint32_t kJumpStamp = 0x40000000u;   // k_jump_keep `level` (wide): word 7 of the child = its own lo (the levels up to K); else the parent's word 7
// k_jump_insert `nb`: the buckets (below 2^32) and, for wide records, K at bits 32..39 and K2 at bits 40..47 (K = 0: narrow records;
// K2 = 0: the key of level 1, the record's first chunk; else the key of level 2, formed from the record)
inline uint64_t jump_insert_nb(uint64_t nb, uint32_t K, uint32_t K2) { return nb | (static_cast<uint64_t>(K) << 32) | (static_cast<uint64_t>(K2) << 40); }

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

// the children that occur go to the next level: {lo, hi, parent key + symbol `level`} appended at *count (one atomic per wave).
// level & kJumpWide: wide records (above) -- the symbol goes to position `level` & 0xFFFF of the record's 112, word 7 is the child's lo
// (kJumpStamp) or the parent's word 7.
__global__ __launch_bounds__(256) void k_jump_keep(const uint64_t *__restrict__ nlo, const uint64_t *__restrict__ nhi, const uint4 *__restrict__ pkey,
                                                   const uint64_t base, const uint64_t N, const uint32_t level, uint64_t *__restrict__ olo,
                                                   uint64_t *__restrict__ ohi, uint4 *__restrict__ okey, unsigned long long *__restrict__ count) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const bool wide = (level & kJumpWide) != 0;
    const uint32_t pos = level & 0xFFFFu;
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
            const uint64_t par = base + (j >> 2);
            olo[o] = nlo[j];
            ohi[o] = nhi[j];
            if (!wide) {
                uint4 kk = pkey[par];
                JumpKey key{{kk.x, kk.y, kk.z, kk.w}};
                jump_key_set(key, pos, static_cast<uint32_t>(j & 3u));
                okey[o] = make_uint4(key.w[0], key.w[1], key.w[2], key.w[3]);
            } else {
                const uint4 a = pkey[2 * par], b = pkey[2 * par + 1];
                JumpKey ka{{a.x, a.y, a.z, a.w}}, kb{{b.x, b.y, b.z, b.w}};
                if (pos < 64u) jump_key_set(ka, pos, static_cast<uint32_t>(j & 3u));
                else jump_key_set(kb, pos - 64u, static_cast<uint32_t>(j & 3u));
                if (level & kJumpStamp) kb.w[3] = static_cast<uint32_t>(nlo[j]);
                okey[2 * o] = make_uint4(ka.w[0], ka.w[1], ka.w[2], ka.w[3]);
                okey[2 * o + 1] = make_uint4(kb.w[0], kb.w[1], kb.w[2], kb.w[3]);
            }
        }
    }
}

// the final level's words as packed reads of K symbols: one 16-byte chunk each (the keys are the chunks), or -- K & kJumpWide -- the two
// chunks of a wide record
__global__ __launch_bounds__(256) void k_jump_meta(const uint64_t cnt, const uint32_t K, uint2 *__restrict__ meta) {
    const uint32_t per = (K & kJumpWide) ? 2u : 1u, len = K & 0xFFFFu;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < cnt; i += stride)
        meta[i] = make_uint2(static_cast<uint32_t>(per * i), len);
}

// insert the searched words: claim a slot by its tag, then write key and state.  nb = jump_insert_nb(buckets, K, K2): narrow records are
// the keys; a wide record gives the key of level 1 (its first chunk: the K symbols, nothing above them yet) or that of level 2 (the K2
// symbols from symbol K on, and word 7).
__global__ __launch_bounds__(256) void k_jump_insert(const uint4 *__restrict__ keys, const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi,
                                                     const uint64_t *__restrict__ ss, const uint64_t cnt, uint32_t *__restrict__ tab, const uint64_t nb_k,
                                                     unsigned long long *__restrict__ inserted) {
    const uint64_t nb = nb_k & 0xFFFFFFFFull;
    const uint32_t K = static_cast<uint32_t>(nb_k >> 32) & 0xFFu, K2 = static_cast<uint32_t>(nb_k >> 40) & 0xFFu;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < cnt; i += stride) {
        const uint64_t l = lo[i], h = hi[i], k = ss ? ss[i] : 0;
        if (l > h || h > 0xFFFFFFFFull) continue;
        uint32_t kk;
        if (k == ~uint64_t(0)) kk = 0xFFFFFFFFu;                  // (as ftab_lookup: the word's last row is text position 0)
        else if (k >= 0xFFFFFFF0ull) continue;                     // not expressible: the read takes the ftab path
        else kk = static_cast<uint32_t>(k);
        uint4 kw = keys[K ? 2 * i : i];
        if (K2) {
            const uint4 b = keys[2 * i + 1];
            const uint32_t f[7] = {kw.x, kw.y, kw.z, kw.w, b.x, b.y, b.z};
            const auto word = [&](const uint32_t j) {             // (selects over static indexes: nothing goes to scratch; words from 7 on hold no symbol)
                uint32_t v = 0;
#pragma unroll
                for (uint32_t t = 0; t < 7; ++t) v = t == j ? f[t] : v;
                return v;
            };
            const JumpKey k2 = jump2_key_from_codes(word, K, K2, b.w);
            kw = make_uint4(k2.w[0], k2.w[1], k2.w[2], k2.w[3]);
        }
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

// *retry: a build with a level 2 outgrew the budget before the first table stood (nothing is built; every scratch is freed on return)
static int build_jump(const DevIndex &ix, const LaunchCfg &cfg, uint32_t K, uint64_t table_budget, uint64_t peak_budget, void **tab,
                      uint64_t *tab_bytes, uint64_t *buckets, uint64_t *keys, const char **why, void *stream, uint32_t K2, uint64_t both_budget,
                      JumpLevel2 *l2, bool *retry, uint64_t *words) {
    *tab = nullptr; *tab_bytes = 0; *buckets = 0; *keys = 0; *words = 0; *why = nullptr;
    if (l2) *l2 = JumpLevel2{};
    if (!l2) K2 = 0;
    if (ix.pos_bytes != 4) { *why = "8-byte positions (the table holds 4-byte states)"; return 0; }
    if (ix.layout != 2 || ix.nmajor != 4 || !ix.stage_ok) { *why = "only the staged search of the run-indexed layout over four major symbols uses it"; return 0; }
    if (K < kJumpMinK || K > kJumpMaxK) return static_cast<int>(hipErrorInvalidValue);
    if (K2 && (K2 < kJump2MinK || K2 > kJump2MaxK)) return static_cast<int>(hipErrorInvalidValue);
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevIndex plain = ix;   // the words are searched WITHOUT a jump table, of either level
    plain.jump = nullptr;
    plain.jump_buckets = 0;
    plain.jump_k = 0;
    plain.jump2_buckets = 0;
    plain.jump2_k = 0;
    plain.jump_complete = 0;
    // a build with a level 2 that outgrows the budget before the first table stands starts again without it: level 1 is decided as if there were no level 2
    auto again_without_level2 = [&]() { *retry = true; return 0; };
    const bool wide = K2 != 0;
    const uint64_t wbytes = wide ? 48 : 32, kq = wide ? 2 : 1;   // bytes of a word {lo, hi, record}; uint4 of a record
    const uint32_t wflag = wide ? kJumpWide : 0u;
    // scratch: two levels of {lo, hi, key} (32 bytes a word; 48 with wide records) and one pass of children (4 C x 33 bytes); the pass takes at most
    // a quarter of `peak_budget`, and every allocation is checked against it BEFORE it is made (scratch + tables never exceed it)
    uint64_t C = kJumpChunkParents;
    while (C > (uint64_t(1) << 12) && 4 * C * 33 > peak_budget / 4) C >>= 1;
    if (4 * C * 33 + 1024 > peak_budget) { *why = "its build scratch exceeds what the HBM budget leaves"; return 0; }
    DevBuf clo, chi, nlo, nhi, sym, mb, cnt_d;
    DevBuf lv_lo[2], lv_hi[2], lv_key[2];
    uint64_t held = 0;   // level 2: the bytes of the first table, which the budget holds already
    uint64_t cap[2] = {0, 0};
    hipError_t e = hipSuccess;
    auto scratch = [&]() {
        return clo.bytes + chi.bytes + nlo.bytes + nhi.bytes + sym.bytes + wbytes * (cap[0] + cap[1]);
    };
    bool over = false;   // set by grow: the larger level would not fit peak_budget (nothing allocated)
    auto grow = [&](int w, uint64_t need, uint64_t used) -> hipError_t {   // level w holds `used` words; make room for `need`
        if (need <= cap[w]) return hipSuccess;
        const uint64_t nc = std::max<uint64_t>(need, cap[w] + cap[w] / 2);
        if (held + scratch() + wbytes * nc > peak_budget) { over = true; return hipSuccess; }   // (old and new level side by side while copying)
        DevBuf a, b, c;
        hipError_t r = a.alloc(nc * 8);
        if (r == hipSuccess) r = b.alloc(nc * 8);
        if (r == hipSuccess) r = c.alloc(nc * 16 * kq);
        if (r == hipSuccess && used) r = hipMemcpyAsync(a.p, lv_lo[w].p, used * 8, hipMemcpyDeviceToDevice, st);
        if (r == hipSuccess && used) r = hipMemcpyAsync(b.p, lv_hi[w].p, used * 8, hipMemcpyDeviceToDevice, st);
        if (r == hipSuccess && used) r = hipMemcpyAsync(c.p, lv_key[w].p, used * 16 * kq, hipMemcpyDeviceToDevice, st);
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
    if (e == hipSuccess && over) {
        if (wide) return again_without_level2();
        *why = "its build scratch exceeds what the HBM budget leaves";
        return 0;
    }
    if (e == hipSuccess) {   // level 0: the empty word, full_range() (rowbowt.hpp:115-118)
        const uint64_t lo0 = 0, hi0 = ix.n - 1;
        const uint4 k0[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
        e = hipMemcpy(lv_lo[0].p, &lo0, 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(lv_hi[0].p, &hi0, 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(lv_key[0].p, k0, 16 * kq, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) return static_cast<int>(e);
    uint64_t F = 1;
    int cur = 0;
    // the symbols [first, last) on every word of the frontier.  Returns a HIP error, or 0 with `over` set when a level would not fit the budget.
    // Wide records: up to K every child is stamped with its own lo, so that the K-mers of the frontier carry theirs; beyond K it travels unchanged.
    auto extend = [&](const uint32_t first, const uint32_t last) -> int {
        for (uint32_t level = first; level < last; ++level) {
            const int nx = cur ^ 1;
            const unsigned long long zero = 0;
            if ((e = hipMemcpy(cnt_d.p, &zero, sizeof(zero), hipMemcpyHostToDevice)) != hipSuccess) return static_cast<int>(e);
            uint64_t used = 0;
            for (uint64_t base = 0; base < F; base += C) {
                const uint64_t cnt = std::min<uint64_t>(C, F - base);
                if ((e = grow(nx, used + 4 * cnt, used)) != hipSuccess) return static_cast<int>(e);
                if (over) return 0;
                hipLaunchKernelGGL(k_jump_expand, dim3(grid_for(cfg, 4 * cnt)), dim3(256), 0, st, lv_lo[cur].as<uint64_t>(), lv_hi[cur].as<uint64_t>(), base, cnt,
                                   mb.as<uint8_t>(), clo.as<uint64_t>(), chi.as<uint64_t>(), sym.as<uint8_t>());
                if ((e = hipGetLastError()) != hipSuccess) return static_cast<int>(e);
                if (int rc = launch_lf(plain, cfg, clo.as<uint64_t>(), chi.as<uint64_t>(), sym.as<uint8_t>(), 4 * cnt, nlo.as<uint64_t>(), nhi.as<uint64_t>(), st)) return rc;
                hipLaunchKernelGGL(k_jump_keep, dim3(grid_for(cfg, 4 * cnt)), dim3(256), 0, st, nlo.as<uint64_t>(), nhi.as<uint64_t>(), lv_key[cur].as<uint4>(), base,
                                   4 * cnt, level | wflag | (wide && level < K ? kJumpStamp : 0u), lv_lo[nx].as<uint64_t>(), lv_hi[nx].as<uint64_t>(),
                                   lv_key[nx].as<uint4>(), cnt_d.as<unsigned long long>());
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
        return 0;
    };
    if (int rc = extend(0, K)) return rc;
    if (over) {
        if (wide) return again_without_level2();
        *why = "its build scratch exceeds what the HBM budget leaves";
        return 0;
    }
    *keys = F;
    *words = F;
    const uint64_t nb = jump_buckets_for(F);
    const uint64_t bytes = nb * kJumpBucketBytes;
    if (F == 0 || nb >= (uint64_t(1) << 32)) { *why = F ? "more keys than the table addresses" : "no K-mer occurs"; return 0; }
    if (bytes > table_budget) {
        *why = "the table exceeds the bytes allowed for it (what the HBM budget leaves; by default also half the replica)";
        return 0;
    }
    if (bytes + scratch() > peak_budget) {
        if (wide) return again_without_level2();
        *why = "the table exceeds the bytes allowed for it (what the HBM budget leaves; by default also half the replica)";
        return 0;
    }
    void *t = nullptr;
    if ((e = hipMalloc(&t, bytes)) != hipSuccess) { (void)hipGetLastError(); *why = "hipMalloc of the table failed"; return 0; }
    // the words of the frontier [0, F), searched as packed reads (their records are the chunks) by the search kernel itself and inserted into
    // `table`; passes of 4 C words in the children's scratch: meta in clo, lo / hi / toehold in chi / nlo / nhi
    unsigned long long ins = 0;
    auto fill = [&](void *table, const uint64_t nbt, const uint32_t len, const uint32_t k2) -> int {
        int rc = static_cast<int>(hipMemsetAsync(table, 0, nbt * kJumpBucketBytes, st));
        if (!rc) rc = static_cast<int>(hipMemsetAsync(cnt_d.p, 0, sizeof(unsigned long long), st));
        for (uint64_t base = 0; !rc && base < F; base += 4 * C) {
            const uint64_t cnt = std::min<uint64_t>(4 * C, F - base);
            const uint4 *recs = lv_key[cur].as<uint4>() + kq * base;
            hipLaunchKernelGGL(k_jump_meta, dim3(grid_for(cfg, cnt)), dim3(256), 0, st, cnt, len | wflag, clo.as<uint2>());
            rc = static_cast<int>(hipGetLastError());
            if (!rc) rc = launch_find_range_runs_packed(plain, cfg, clo.as<uint2>(), recs, cnt, chi.as<uint64_t>(), nlo.as<uint64_t>(),
                                                        ix.has_tsa ? nhi.as<uint64_t>() : nullptr, st);
            if (!rc) {
                hipLaunchKernelGGL(k_jump_insert, dim3(grid_for(cfg, cnt)), dim3(256), 0, st, recs, chi.as<uint64_t>(), nlo.as<uint64_t>(),
                                   ix.has_tsa ? nhi.as<uint64_t>() : nullptr, cnt, static_cast<uint32_t *>(table), jump_insert_nb(nbt, wide ? K : 0u, k2),
                                   cnt_d.as<unsigned long long>());
                rc = static_cast<int>(hipGetLastError());
            }
        }
        if (!rc) rc = static_cast<int>(hipMemcpyAsync(&ins, cnt_d.p, sizeof(ins), hipMemcpyDeviceToHost, st));
        if (!rc) rc = static_cast<int>(hipStreamSynchronize(st));
        return rc;
    };
    if (int rc = fill(t, nb, K, 0)) { (void)hipFree(t); return rc; }
    *tab = t;
    *tab_bytes = bytes;
    *buckets = nb;
    *keys = ins;
    if (!wide) return 0;

    // ---- level 2: K2 more symbols on every K-mer; the words of K + K2 symbols searched and inserted under their level-2 keys.  It is the last thing the
    // budget pays for: a budget or a device memory that runs out leaves the first table and no second (l2->why); any other error fails the build as a whole.
    const auto t2_0 = std::chrono::steady_clock::now();
    held = bytes;
    auto give_up = [&](const char *w) { (void)hipGetLastError(); l2->why = w; return 0; };
    auto fail2 = [&](int err) {
        if (err == static_cast<int>(hipErrorOutOfMemory)) return give_up("out of device memory while building it");
        (void)hipFree(t);
        *tab = nullptr; *tab_bytes = 0; *buckets = 0;
        return err;
    };
    if (int err = extend(K, K + K2)) return fail2(err);
    if (over) return give_up("its build scratch exceeds what the HBM budget leaves");
    l2->keys = F;
    l2->words = F;
    const uint64_t nb2 = jump_buckets_for(F);
    const uint64_t bytes2 = nb2 * kJumpBucketBytes;
    if (F == 0 || nb2 >= (uint64_t(1) << 32)) return give_up(F ? "more keys than the table addresses" : "no word of K + K2 symbols occurs");
    // The two tables are ONE allocation, the second behind the first (DevIndex names the first; a replica copies and re-points one array): the
    // first table moves into it before it is published, so for a moment the budget holds it twice.
    if (held + bytes2 > both_budget || 2 * held + bytes2 + scratch() > peak_budget)
        return give_up("the table exceeds the bytes allowed for it (what the HBM budget leaves after the first table; by default both together at most the replica)");
    void *tc = nullptr;
    if (hipMalloc(&tc, bytes + bytes2) != hipSuccess) return give_up("hipMalloc of the table failed");
    hipError_t ce = hipMemcpyAsync(tc, t, bytes, hipMemcpyDeviceToDevice, st);
    if (ce == hipSuccess) ce = hipStreamSynchronize(st);
    if (ce != hipSuccess) { (void)hipFree(tc); return fail2(static_cast<int>(ce)); }
    (void)hipFree(t);
    t = tc;
    *tab = tc;
    void *t2 = static_cast<char *>(tc) + bytes;
    if (int rc = fill(t2, nb2, K + K2, K2)) {   // (after the move the allocation is larger than the first table's record of it: no half measures)
        (void)hipFree(t);
        *tab = nullptr; *tab_bytes = 0; *buckets = 0;
        return rc;
    }
    l2->tab = t2;
    l2->bytes = bytes2;
    l2->buckets = nb2;
    l2->keys = ins;
    l2->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2_0).count();
    return 0;
}

int launch_build_jump(const DevIndex &ix, const LaunchCfg &cfg, uint32_t K, uint64_t table_budget, uint64_t peak_budget, void **tab,
                      uint64_t *tab_bytes, uint64_t *buckets, uint64_t *keys, const char **why, void *stream, uint32_t K2, uint64_t both_budget,
                      JumpLevel2 *l2, uint64_t *words) {
    bool retry = false;
    uint64_t words1 = 0;
    if (!words) words = &words1;
    int rc = build_jump(ix, cfg, K, table_budget, peak_budget, tab, tab_bytes, buckets, keys, why, stream, K2, both_budget, l2, &retry, words);
    if (!retry) return rc;
    rc = build_jump(ix, cfg, K, table_budget, peak_budget, tab, tab_bytes, buckets, keys, why, stream, 0, 0, nullptr, &retry, words);
    l2->why = "its build scratch exceeds what the HBM budget leaves";
    return rc;
}

}  // namespace rbg
