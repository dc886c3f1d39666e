// rbg_sam_dev.hpp -- what the SAM kernels of k_sam.hip and sam_extend.hip share: the batch as a kernel sees it, the parts of a line, the body of the write
// kernels (kSamLines lines per workgroup formatted into LDS at their offsets, the workgroup's stretch leaving in aligned 16-byte stores; a stretch
// longer than kSamLds goes straight to memory, lane by lane), the workspace's layout.  `ext` (nullable): one SamExtend per line -- the extended lines of
// rbg_align_sam_extend; nullptr gives rbg_align_sam's lines; `ext_right` (nullable, with ext): the lines' right extensions (fl_extend.hip).  Everything lives in an anonymous namespace: each unit gets its own inlined copy.
#pragma once

#include "rbg_device.hpp"
#include "rbg_sam.hpp"

namespace rbg {
namespace {

constexpr uint32_t kSamGridCap = 4096;     // workgroups per launch, at most

struct SamArgs {
    uint64_t N, E;                                  // reads, lines
    const uint64_t *lo, *hi, *a, *b;                // [N] the picked seed (unmapped: lo = 1, hi = 0)
    const uint8_t *rev;                             // [N]
    const uint64_t *line_off, *loc_off, *locs;      // [N + 1], [N + 1], [loc_off[N]]
    const char *seqs, *quals;                       // the reads' original bytes; quals nullable, same offsets
    const uint64_t *roff;                           // [N + 1]
    const char *names;
    const uint32_t *name_off;                       // [N + 1]
    const uint64_t *doc_start;                      // [ndocs] sorted
    const char *doc_names;
    const uint32_t *doc_name_off;                   // [ndocs + 1]
    uint64_t ndocs, text_size;
};

inline int sam_grid(const uint64_t work, const uint32_t per_block, const uint32_t cap_arg) {
    const uint64_t cap = cap_arg ? cap_arg : kSamGridCap;
    const uint64_t g = (work + per_block - 1) / per_block;
    return static_cast<int>(std::max<uint64_t>(1, std::min(g, cap)));
}

// k_text.hip's doc_of: the number of sorted starts below min(pos + 1, size); 0: no document
__device__ __forceinline__ uint64_t sam_doc_of(const SamArgs &s, const uint64_t pos) {
    const uint64_t q = pos + 1 > s.text_size ? s.text_size : pos + 1;
    uint64_t lo = 0, hi = s.ndocs;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (s.doc_start[mid] < q) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the parts of line e of read i (d: its document, for a mapped line)
__device__ __forceinline__ SamLine sam_line_of(const SamArgs &s, const uint64_t e, const uint64_t i, const uint32_t d) {
    SamLine L;
    L.name_len = s.name_off[i + 1] - s.name_off[i];
    L.mapped = s.hi[i] >= s.lo[i];
    L.reverse = s.rev[i] != 0;
    L.hit = e - s.line_off[i] + 1;
    L.occ = s.hi[i] - s.lo[i] + 1;
    L.m = s.roff[i + 1] - s.roff[i];
    L.a = s.a[i];
    L.b = s.b[i];
    L.has_qual = s.quals != nullptr;
    L.rname_len = 0;
    L.pos = 0;
    if (L.mapped) {
        const uint64_t pos = s.locs[s.loc_off[i] + (L.hit - 1)];
        L.rname_len = s.doc_name_off[d + 1] - s.doc_name_off[d];
        L.pos = pos - s.doc_start[d] + 1;
    }
    return L;
}

__device__ __forceinline__ void sam_put(const SamArgs &s, const uint64_t e, const uint64_t i, const uint32_t d, char *p, const SamExtend *ext,
                                        const SamExtend *ext_right = nullptr) {
    const SamLine L = sam_line_of(s, e, i, d);
    sam_put_line(p, L, s.names + s.name_off[i], s.doc_names + s.doc_name_off[d], s.seqs + s.roff[i], s.quals ? s.quals + s.roff[i] : nullptr,
                 ext && L.mapped ? ext + e : nullptr, ext && ext_right && L.mapped ? ext_right + e : nullptr);
}

// the body of k_sam_write: kSamLines lines per workgroup (= its threads), s_buf its kSamLds + 16 bytes of LDS, 16-byte aligned (the including unit's constants)
template <uint32_t kSamLines, uint32_t kSamLds>
__device__ __forceinline__ void sam_write_lines(const SamArgs &s, const uint32_t *__restrict__ eread, const uint32_t *__restrict__ doc, const uint64_t *__restrict__ at,
                                                const uint64_t total, char *__restrict__ text, char *s_buf, const SamExtend *__restrict__ ext,
                                                const SamExtend *__restrict__ ext_right = nullptr) {
    const uint64_t nblocks = (s.E + kSamLines - 1) / kSamLines;
    for (uint64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const uint64_t e0 = blk * kSamLines, e1 = e0 + kSamLines < s.E ? e0 + kSamLines : s.E;
        const uint64_t t0 = at[e0], t1 = e1 < s.E ? at[e1] : total;
        const uint64_t e = e0 + threadIdx.x;
        const uint32_t shift = static_cast<uint32_t>((reinterpret_cast<uintptr_t>(text) + t0) & 15u);   // LDS and memory addresses congruent mod 16
        if (t1 - t0 <= kSamLds) {
            if (e < e1) sam_put(s, e, eread[e], doc[e], s_buf + shift + (at[e] - t0), ext, ext_right);
            __syncthreads();
            const uint32_t nbytes = static_cast<uint32_t>(t1 - t0);
            char *dst = text + t0;
            const char *src = s_buf + shift;
            const uint32_t head = (16u - shift) & 15u;                      // bytes before the first 16-byte boundary
            const uint32_t h = head < nbytes ? head : nbytes;
            if (threadIdx.x < h) dst[threadIdx.x] = src[threadIdx.x];
            const uint32_t body = (nbytes - h) >> 4;
            for (uint32_t j = threadIdx.x; j < body; j += kSamLines)
                reinterpret_cast<uint4 *>(dst + h)[j] = reinterpret_cast<const uint4 *>(src + h)[j];
            const uint32_t done = h + (body << 4);
            if (threadIdx.x < nbytes - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
            __syncthreads();
        } else if (e < e1) {
            sam_put(s, e, eread[e], doc[e], text + at[e], ext, ext_right);  // (a long name or read: straight to memory, byte by byte)
        }
    }
}

inline size_t up256(size_t x) { return (x + 255) & ~size_t(255); }
// the workspace: eread / doc (4 bytes per line), len / at (8), the scans' temporaries (tmp_bytes: k_sam.hip sam_scan_bytes)
struct SamWs {
    uint32_t *eread, *doc;
    uint64_t *len, *at;
    void *tmp;
    size_t tmp_bytes;
};
inline SamWs sam_ws_ptrs(void *ws, uint64_t E) {
    char *b = static_cast<char *>(ws);
    SamWs w;
    w.eread = reinterpret_cast<uint32_t *>(b);
    w.doc = reinterpret_cast<uint32_t *>(b + up256(E * 4));
    w.len = reinterpret_cast<uint64_t *>(b + 2 * up256(E * 4));
    w.at = reinterpret_cast<uint64_t *>(b + 2 * up256(E * 4) + up256(E * 8));
    w.tmp = b + 2 * up256(E * 4) + 2 * up256(E * 8);
    w.tmp_bytes = 0;
    return w;
}

inline SamArgs sam_args(const SamBatch &B) {
    return SamArgs{B.N, B.E, B.lo, B.hi, B.a, B.b, B.rev, B.line_off, B.loc_off, B.locs, B.seqs, B.quals, B.roff, B.names, B.name_off,
                   B.doc_start, B.doc_names, B.doc_name_off, B.ndocs, B.text_size};
}

}  // namespace
}  // namespace rbg
