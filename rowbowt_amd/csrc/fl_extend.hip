// fl_extend.hip -- FL over the run lists of the BWT (rbg_fl_dev), the right extension of located seeds by an FL walk (rbg_extend_right_dev) and the SAM lines
// extended on both sides of rbg_align_sam_extend_both (include/rbg.h; the structure and its step: rbg_fl.hpp; the rule of the walk and of the lines: rbg_sam.hpp).
// Templated on the position width only: the FL index does not depend on the rank layout.
//
//   k_fl_rows          one lane per row, grid-stride: sym[j] = the row's F byte (0 when it is not one of A C G T), next[j] = FL(row) (2^64 - 1 then)
//   k_extend_right     one lane per item {sequence, b, row, skip, limit}, grid-stride: the lane takes `skip` FL steps without comparing (they cross the seed),
//                      then reads the reference base right of the seed as the F symbol of its row and steps row = FL(row), comparing with the read's
//                      clipped suffix, until rbg_sam.hpp's rule ends the walk; one SamExtend per item, t counted rightwards.  An FL step is a dependent
//                      pair of gathers -- the directory pair, then the bucket's first two entries --, a third only in a bucket of three or more runs.
//   k_sam_right_items  per output line of rbg_align_sam_extend_both that has a right clip: the item of its walk and its budget (K - the left walk's nm);
//                      every other line is marked as having none and costs no walk
//   k_sam_len_both / k_sam_write_both
//                      k_sam.hip's length and write kernels with both extension records of every line (rbg_sam_dev.hpp: the same bodies, the same staging)
//
// As in k_extend_left the walk's state stays in registers and each taken mismatch is written straight into the record: no scratch.  The FlView is staged
// in LDS: a lane picks its base's lists by an index, and indexing kernel arguments by a lane value would put them in scratch.
#include "rbg_fl.hpp"
#include "rbg_launch.hpp"
#include "rbg_sam_dev.hpp"

namespace rbg {
namespace {

constexpr uint32_t kSamLines = 128;        // lines per workgroup of k_sam_write_both (= its threads): k_sam.hip's
constexpr uint32_t kSamLds = 48 * 1024;    // bytes of text a workgroup stages: k_sam.hip's
constexpr uint32_t kNoItem = 0xFFFFFFFFu;  // item_seq of a line without a walk (only the lines' own items carry it: they come with budgets)

static_assert(sizeof(SamExtend) == 56 && RBG_SAM_MAX_MISMATCH == 8, "include/rbg.h rbg_extend_t");

struct RightItems {
    const uint32_t *seq, *b, *skip;    // [M] the sequence of the batch, the seed's end in it, the FL steps that cross the seed
    const uint64_t *row, *limit;       // [M] the row of the seed's first base, and how far right of the seed the walk may go
    const uint32_t *k;                 // [M] nullable: the item's own budget (the lines'); else the launch's
    uint64_t M;
};

template <typename P>
__global__ __launch_bounds__(256) void k_fl_rows(const FlView v, const uint64_t n, const uint64_t *__restrict__ rows, const uint64_t M, uint8_t *__restrict__ sym,
                                                 uint64_t *__restrict__ next, unsigned int *__restrict__ err) {
    __shared__ FlView s_v;
    if (threadIdx.x == 0) s_v = v;
    __syncthreads();
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < M; i += stride) {
        const uint64_t r = rows[i];
        if (r >= n) {
            sym[i] = 0;
            next[i] = 0;
            atomicOr(err, 1u);
            continue;
        }
        const FlStep st = fl_step<P>(s_v, r);
        sym[i] = static_cast<uint8_t>(st.sym);
        next[i] = st.next;
    }
}

template <typename P>
__global__ __launch_bounds__(256) void k_extend_right(const FlView v, const uint64_t n, const uint8_t *__restrict__ seqs, const uint64_t *__restrict__ off,
                                                      const uint64_t N, const RightItems it, const uint32_t K, SamExtend *__restrict__ out,
                                                      unsigned int *__restrict__ err) {
    __shared__ FlView s_v;
    if (threadIdx.x == 0) s_v = v;
    __syncthreads();
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < it.M; i += stride) {
        const uint32_t sq = it.seq[i];
        uint32_t *words = reinterpret_cast<uint32_t *>(out + i);
#pragma unroll
        for (uint32_t k = 0; k < sizeof(SamExtend) / 4; ++k) words[k] = 0u;
        if (it.k && sq == kNoItem) continue;            // a line without a right clip: the zero record
        const uint64_t b = it.b[i], r0 = it.row[i], lim = it.limit[i];
        const uint32_t skip = it.skip[i];
        uint64_t base = 0, m = 0;
        bool bad = sq >= N || r0 >= n || skip > b;
        if (!bad) {
            base = off[sq];
            m = off[sq + 1] - base;
            bad = b > m;
        }
        if (bad) { atomicOr(err, 1u); continue; }       // (the record stays zero)
        uint64_t r = r0;
        bool live = true;
        for (uint32_t s = 0; s < skip; ++s) {           // across the seed: no base on the way ends the item with a zero extension
            const FlStep st = fl_step<P>(s_v, r);
            if (!st.sym) { live = false; break; }
            r = st.next;
        }
        if (!live) continue;
        SamExtendWalk w = sam_extend_begin(m - b, lim, it.k ? it.k[i] : K);
        ByteCursor rd{reinterpret_cast<const uint4 *>(seqs), ~uint64_t(0), make_uint4(0, 0, 0, 0)};
        while (w.t < w.L) {
            const FlStep st = fl_step<P>(s_v, r);       // the reference base at this row, and the row one base further right
            const uint32_t x = rd.at(base + b + w.t);
            bool mismatch;
            if (!sam_extend_take(w, st.sym, x, &mismatch)) break;
            if (mismatch) {
                out[i].mis_t[w.mm - 1] = w.t - 1;
                out[i].mis_ref[w.mm - 1] = static_cast<uint8_t>(st.sym);
            }
            r = st.next;
        }
        out[i].ext = w.e;
        out[i].nm = w.nm;
        out[i].score = w.best;
        out[i].steps = w.steps;
    }
}

__global__ __launch_bounds__(256) void k_sam_right_items(const SamArgs s, const uint32_t *__restrict__ eread, const uint32_t *__restrict__ doc,
                                                         const SamExtend *__restrict__ left, const uint64_t n, const uint32_t K, uint32_t *__restrict__ item_seq,
                                                         uint32_t *__restrict__ item_b, uint64_t *__restrict__ item_row, uint32_t *__restrict__ item_skip,
                                                         uint64_t *__restrict__ item_limit, uint32_t *__restrict__ item_k) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < s.E; e += stride) {
        const uint64_t i = eread[e];
        uint32_t sq = kNoItem, b32 = 0, skip = 0, k = 0;
        uint64_t row = 0, limit = 0;
        if (s.hi[i] >= s.lo[i]) {
            const uint64_t m = s.roff[i + 1] - s.roff[i], a = s.a[i], b = s.b[i];
            if (m > b) {
                const uint64_t j = e - s.line_off[i], pos = s.locs[s.loc_off[i] + j], d = doc[e];
                const uint64_t doc_end = d + 1 < s.ndocs ? s.doc_start[d + 1] : n, seed_end = pos + (b - a);
                if (doc_end > seed_end) {                // (a seed over a document boundary: nothing right of it belongs to the line's document)
                    sq = static_cast<uint32_t>(2 * i + (s.rev[i] ? 1 : 0));
                    b32 = static_cast<uint32_t>(b);
                    skip = static_cast<uint32_t>(b - a);
                    row = s.hi[i] - j;
                    limit = doc_end - seed_end;
                    const uint32_t used = left[e].nm;
                    k = K > used ? K - used : 0u;
                }
            }
        }
        item_seq[e] = sq;
        item_b[e] = b32;
        item_row[e] = row;
        item_skip[e] = skip;
        item_limit[e] = limit;
        item_k[e] = k;
    }
}

__global__ __launch_bounds__(256) void k_sam_len_both(const SamArgs s, const uint32_t *__restrict__ eread, const uint32_t *__restrict__ doc,
                                                      const SamExtend *__restrict__ ext, const SamExtend *__restrict__ ext_right, uint64_t *__restrict__ len) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < s.E; e += stride) {
        const SamLine L = sam_line_of(s, e, eread[e], doc[e]);
        len[e] = sam_line_len(L, L.mapped ? ext + e : nullptr, L.mapped ? ext_right + e : nullptr);
    }
}

__global__ __launch_bounds__(kSamLines) void k_sam_write_both(const SamArgs s, const uint32_t *__restrict__ eread, const uint32_t *__restrict__ doc,
                                                              const uint64_t *__restrict__ at, const uint64_t total, char *__restrict__ text,
                                                              const SamExtend *__restrict__ ext, const SamExtend *__restrict__ ext_right) {
    __shared__ __align__(16) char s_buf[kSamLds + 16];
    sam_write_lines<kSamLines, kSamLds>(s, eread, doc, at, total, text, s_buf, ext, ext_right);
}

}  // namespace

int launch_fl_rows(const FlView &v, uint32_t pos_bytes, uint64_t n, const uint64_t *rows, uint64_t M, uint8_t *sym, uint64_t *next, unsigned int *d_err,
                   uint32_t cap, void *stream) {
    if (M == 0) return 0;
    const dim3 grid(sam_grid(M, 256, cap)), block(256);
    return with_pos(pos_bytes, [&](auto p) { return launch_grid(k_fl_rows<pos_t<decltype(p)>>, grid, block, 0, stream, v, n, rows, M, sym, next, d_err); });
}

int launch_extend_right(const FlView &v, uint32_t pos_bytes, uint64_t n, const uint8_t *seqs, const uint64_t *off, uint64_t N, const uint32_t *item_seq,
                        const uint32_t *item_b, const uint64_t *item_row, const uint32_t *item_skip, const uint64_t *item_limit, const uint32_t *item_k, uint64_t M,
                        uint32_t max_mismatch, void *out, unsigned int *d_err, uint32_t cap, void *stream) {
    if (M == 0) return 0;
    if (max_mismatch > RBG_SAM_MAX_MISMATCH) return static_cast<int>(hipErrorInvalidValue);
    const RightItems it{item_seq, item_b, item_skip, item_row, item_limit, item_k, M};
    const dim3 grid(sam_grid(M, 256, cap)), block(256);
    SamExtend *o = static_cast<SamExtend *>(out);
    return with_pos(pos_bytes, [&](auto p) {
        return launch_grid(k_extend_right<pos_t<decltype(p)>>, grid, block, 0, stream, v, n, seqs, off, N, it, max_mismatch, o, d_err);
    });
}

// rbg_align_sam_extend_both after the left walks: the right items of the lines (the workspace holds every line's read and document by then)
int launch_sam_right_items(const SamBatch &B, void *ws, const void *ext_left, uint64_t n, uint32_t K, uint32_t *item_seq, uint32_t *item_b, uint64_t *item_row,
                           uint32_t *item_skip, uint64_t *item_limit, uint32_t *item_k, uint32_t cap, void *stream) {
    const SamWs w = sam_ws_ptrs(ws, B.E);
    return launch_grid(k_sam_right_items, dim3(sam_grid(B.E, 256, cap)), dim3(256), 0, stream, sam_args(B), w.eread, w.doc, static_cast<const SamExtend *>(ext_left), n,
                       K, item_seq, item_b, item_row, item_skip, item_limit, item_k);
}
// the lengths of the lines extended on both sides (launch_sam_offsets, k_sam.hip, turns them into offsets)
int launch_sam_both_len(const SamBatch &B, void *ws, const void *ext, const void *ext_right, uint32_t cap, void *stream) {
    const SamWs w = sam_ws_ptrs(ws, B.E);
    return launch_grid(k_sam_len_both, dim3(sam_grid(B.E, 256, cap)), dim3(256), 0, stream, sam_args(B), w.eread, w.doc, static_cast<const SamExtend *>(ext),
                       static_cast<const SamExtend *>(ext_right), w.len);
}
// the text (total bytes at `text`)
int launch_sam_both_fill(const SamBatch &B, void *ws, const void *ext, const void *ext_right, uint64_t total, char *text, uint32_t cap, void *stream) {
    const SamWs w = sam_ws_ptrs(ws, B.E);
    return launch_grid(k_sam_write_both, dim3(sam_grid(B.E, kSamLines, cap)), dim3(kSamLines), 0, stream, sam_args(B), w.eread, w.doc, w.at, total, text,
                       static_cast<const SamExtend *>(ext), static_cast<const SamExtend *>(ext_right));
}

}  // namespace rbg
