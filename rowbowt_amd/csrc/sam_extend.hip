// sam_extend.hip -- the left extension of located seeds by an LF walk (rbg_extend_left_dev) and the extended SAM lines of rbg_align_sam_extend (include/rbg.h;
// the rule of the walk and of the lines: rbg_sam.hpp).
//
//   k_extend_left    one lane per item {sequence, a, row, limit}, grid-stride: the lane reads the reference base left of its occurrence as BWT[row] and steps
//                    row = LF(row), comparing with the read's clipped prefix, until rbg_sam.hpp's rule ends the walk; one SamExtend per item.
//                    Neither layout stores the BWT by row, so BWT[row] is found with the depth-1 step of the seeding kernels on the one-row range
//                    [row, row]: exactly one of A C G T (or none) leaves it non-empty.  The read's own base is tried first -- on a match that is the step's
//                    only request --, the other three after a miss; a miss that the budget could not take any more is not resolved at all (the walk ends
//                    whatever the base is).  Slot layout: rank_in_slot over the symbol's slots, the three misses' slots loaded before the first is evaluated.
//                    Run-indexed layout: lane_lf2 (rbg_runs2_device.hpp) on the depth-1 table, the lane by itself -- the lanes of a wave are at different
//                    steps of walks of different lengths, there is no step they take together.
//   k_sam_ext_items  per output line of rbg_align_sam_extend: its read (a search of line_off: no mark and scan), its document, and the item of its walk --
//                    line j of the range [lo, hi] is row hi - (j - 1), its limit the location's offset in its document
//   k_sam_len_ext / k_sam_write_ext
//                    k_sam.hip's length and write kernels with the extension record of every line (rbg_sam_dev.hpp: the same bodies, the same staging)
//
// The walk is a dependent chain of gathers like a greedy seed's; the lane keeps its state in registers and writes the mismatches it takes straight into its
// record (an array indexed by the mismatch count would live in scratch).
#include "rbg_runs2_device.hpp"
#include "rbg_launch.hpp"
#include "rbg_sam_dev.hpp"

namespace rbg {
namespace {

constexpr uint32_t kSamLines = 128;        // lines per workgroup of k_sam_write_ext (= its threads): k_sam.hip's
constexpr uint32_t kSamLds = 48 * 1024;    // bytes of text a workgroup stages: k_sam.hip's

static_assert(sizeof(SamExtend) == 56 && RBG_SAM_MAX_MISMATCH == 8, "include/rbg.h rbg_extend_t");

struct ExtendItems {
    const uint32_t *seq, *a;       // [M] the sequence of the batch, the seed's start in it
    const uint64_t *row, *limit;   // [M] the occurrence's row, and how far left it may go (its offset in its document)
    uint64_t M;
};

// A C G T <-> 0 1 3 2
__device__ __forceinline__ uint32_t acgt_index(const uint32_t c) { return (c >> 1) & 3u; }
__device__ __forceinline__ uint32_t acgt_byte(const uint32_t j) { return j == 0 ? 'A' : j == 1 ? 'C' : j == 2 ? 'T' : 'G'; }

// rank_pair (rbg_device.hpp) of the one-row range in two halves, so that several symbols' slots can be in flight together
struct RowSlots {
    RankSlot sl, sh;
    uint64_t bl, bh;
};
__device__ __forceinline__ RowSlots load_row_slots(const DevSym &S, const uint64_t r) {
    const RankSlot *__restrict__ slots = static_cast<const RankSlot *>(S.slots);
    RowSlots x;
    x.bl = r >> S.shift;
    x.bh = (r + 1) >> S.shift;
    x.sl = load_slot(slots + x.bl);
    x.sh = x.sl;
    if (x.bh != x.bl) x.sh = load_slot(slots + x.bh);
    return x;
}
template <typename P>
__device__ __forceinline__ bool row_slots_step(const DevSym &S, const uint8_t *__restrict__ dense, const RowSlots &x, const uint64_t r, uint64_t &nr) {
    RankAux pa, qa;
    const uint64_t c_before = rank_in_slot<P>(S, x.sl, x.bl, r, dense, &pa), c_upto = rank_in_slot<P>(S, x.sh, x.bh, r + 1, dense, &qa);
    if (c_upto <= c_before) return false;
    nr = S.F + c_before;
    return true;
}

template <typename P, bool RUNS>
__global__ __launch_bounds__(256) void k_extend_left(const DevIndex ix, const uint8_t *__restrict__ seqs, const uint64_t *__restrict__ off, const uint64_t N,
                                                     const ExtendItems it, const uint32_t K, SamExtend *__restrict__ out, unsigned int *__restrict__ err) {
    // per base index: the run-indexed layout's depth-1 table, or the slot layout's symbol record; s_have: the index holds the base
    __shared__ uint32_t s_rec[4];
    __shared__ uint32_t s_have[4];
    __shared__ DevSym s_sym[RUNS ? 1 : 4];
    RBG_RUN_SEARCH2_SHARED;
    RunSearch2<P> S2{};
    if constexpr (RUNS) S2 = stage_run_search2<P>(ix, s_tab_first, s_ent2, s_dir2, s_rec2, s_dyn);
    else { (void)s_tab_first; (void)s_ent2; (void)s_dir2; (void)s_rec2; (void)s_dyn; }
    if (threadIdx.x < 4) {
        const uint32_t slot = ix.lut[acgt_byte(threadIdx.x)];
        bool have = slot != 0xFFu;
        if constexpr (RUNS) {
            have = have && slot < static_cast<uint32_t>(kLdsSyms);
            s_rec[threadIdx.x] = have ? run_record(s_tab_first, 1u, slot) : 0u;
        } else {
            s_rec[threadIdx.x] = 0u;
            if (have) s_sym[threadIdx.x] = ix.syms[slot];
        }
        s_have[threadIdx.x] = have ? 1u : 0u;
    }
    __syncthreads();
    // the one-row range [r, r] stepped by base j: true and the new row when BWT[r] is that base
    auto step = [&](const uint32_t j, const uint64_t r, uint64_t &nr) -> bool {
        if (!s_have[j]) return false;
        if constexpr (RUNS) {
            RunStep rs;
            lane_lf2<P>(S2, 0u, s_rec[j], r, r + 1, rs);
            if (rs.c_upto <= rs.c_before) return false;
            nr = rs.F + rs.c_before;
            return true;
        } else {
            const DevSym S = s_sym[j];
            return row_slots_step<P>(S, ix.dense, load_row_slots(S, r), r, nr);
        }
    };
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < it.M; i += stride) {
        const uint32_t sq = it.seq[i];
        const uint64_t a = it.a[i], r0 = it.row[i], lim = it.limit[i];
        uint32_t *words = reinterpret_cast<uint32_t *>(out + i);
#pragma unroll
        for (uint32_t k = 0; k < sizeof(SamExtend) / 4; ++k) words[k] = 0u;
        uint64_t base = 0;
        bool bad = sq >= N || r0 >= ix.n;
        if (!bad) {
            base = off[sq];
            bad = a > off[sq + 1] - base;
        }
        if (bad) { atomicOr(err, 1u); continue; }   // (the record stays zero)
        SamExtendWalk w = sam_extend_begin(a, lim, K);
        ByteCursor rd{reinterpret_cast<const uint4 *>(seqs), ~uint64_t(0), make_uint4(0, 0, 0, 0)};
        uint64_t r = r0;
        while (w.t < w.L) {
            const uint32_t x = rd.at(base + a - 1 - w.t);
            const bool own = sam_is_acgt(x);
            uint32_t c = 0;       // BWT[r] when it is one of A C G T
            uint64_t nr = 0;
            if (own && step(acgt_index(x), r, nr)) {
                c = x;
            } else {
                if (w.mm >= w.K) break;   // (whatever the base is, the budget cannot take it: the rule stops here either way)
                const uint32_t skip = own ? acgt_index(x) : 4u;
                if constexpr (RUNS) {
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) {
                        uint64_t nj = 0;
                        if (j != skip && step(j, r, nj)) { c = acgt_byte(j); nr = nj; }
                    }
                } else {
                    RowSlots rs[4];
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j)
                        if (j != skip && s_have[j]) rs[j] = load_row_slots(s_sym[j], r);
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) {
                        uint64_t nj = 0;
                        if (j != skip && s_have[j] && row_slots_step<P>(s_sym[j], ix.dense, rs[j], r, nj)) { c = acgt_byte(j); nr = nj; }
                    }
                }
            }
            bool mismatch;
            if (!sam_extend_take(w, c, x, &mismatch)) break;
            if (mismatch) {
                out[i].mis_t[w.mm - 1] = w.t - 1;
                out[i].mis_ref[w.mm - 1] = static_cast<uint8_t>(c);
            }
            r = nr;
        }
        out[i].ext = w.e;
        out[i].nm = w.nm;
        out[i].score = w.best;
        out[i].steps = w.steps;
    }
}

__global__ __launch_bounds__(256) void k_sam_ext_items(const SamArgs s, uint32_t *__restrict__ eread, uint32_t *__restrict__ doc, uint32_t *__restrict__ item_seq,
                                                       uint32_t *__restrict__ item_a, uint64_t *__restrict__ item_row, uint64_t *__restrict__ item_limit,
                                                       unsigned int *__restrict__ bad) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < s.E; e += stride) {
        uint64_t lo = 0, hi = s.N - 1;   // the last read whose first line is at or before e (every read has a line)
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo + 1) >> 1);
            if (s.line_off[mid] <= e) lo = mid; else hi = mid - 1;
        }
        const uint64_t i = lo;
        eread[e] = static_cast<uint32_t>(i);
        uint32_t d = 0, sq = 0, a = 0;
        uint64_t row = 0, limit = 0;    // (an unmapped line: the walk of no base)
        if (s.hi[i] >= s.lo[i]) {
            const uint64_t j = e - s.line_off[i], pos = s.locs[s.loc_off[i] + j];
            const uint64_t dj = sam_doc_of(s, pos);
            if (dj == 0) {
                atomicOr(bad, 1u);
            } else {
                d = static_cast<uint32_t>(dj - 1);
                sq = static_cast<uint32_t>(2 * i + (s.rev[i] ? 1 : 0));
                a = static_cast<uint32_t>(s.a[i]);
                row = s.hi[i] - j;
                limit = pos - s.doc_start[d];
            }
        }
        doc[e] = d;
        item_seq[e] = sq;
        item_a[e] = a;
        item_row[e] = row;
        item_limit[e] = limit;
    }
}

__global__ __launch_bounds__(256) void k_sam_len_ext(const SamArgs s, const uint32_t *__restrict__ eread, const uint32_t *__restrict__ doc,
                                                     const SamExtend *__restrict__ ext, uint64_t *__restrict__ len) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < s.E; e += stride) {
        const SamLine L = sam_line_of(s, e, eread[e], doc[e]);
        len[e] = sam_line_len(L, L.mapped ? ext + e : nullptr);
    }
}

__global__ __launch_bounds__(kSamLines) void k_sam_write_ext(const SamArgs s, const uint32_t *__restrict__ eread, const uint32_t *__restrict__ doc,
                                                             const uint64_t *__restrict__ at, const uint64_t total, char *__restrict__ text,
                                                             const SamExtend *__restrict__ ext) {
    __shared__ __align__(16) char s_buf[kSamLds + 16];
    sam_write_lines<kSamLines, kSamLds>(s, eread, doc, at, total, text, s_buf, ext);
}

}  // namespace

int launch_extend_left(const DevIndex &ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, const uint32_t *item_seq, const uint32_t *item_a,
                       const uint64_t *item_row, const uint64_t *item_limit, uint64_t M, uint32_t max_mismatch, void *out, unsigned int *d_err, uint32_t cap,
                       void *stream) {
    if (M == 0) return 0;
    if (max_mismatch > RBG_SAM_MAX_MISMATCH) return static_cast<int>(hipErrorInvalidValue);
    const ExtendItems it{item_seq, item_a, item_row, item_limit, M};
    const dim3 grid(sam_grid(M, 256, cap)), block(256);
    SamExtend *o = static_cast<SamExtend *>(out);
    return with_pos(ix.pos_bytes, [&](auto p) { return with_flag(ix.layout == 2, [&](auto runs) {
        constexpr bool R = decltype(runs)::value;
        return launch_lds(k_extend_left<pos_t<decltype(p)>, R>, grid, block, R ? run_search2_lds(ix) : 0, 1024, stream, ix, seqs, off, N, it, max_mismatch, o, d_err);
    }); });
}

// phase 1 of rbg_align_sam_extend's text: every line's read and document into the workspace (sam_ws_bytes(E)), the items of the lines' walks
int launch_sam_ext_items(const SamBatch &B, void *ws, uint32_t *item_seq, uint32_t *item_a, uint64_t *item_row, uint64_t *item_limit, unsigned int *d_bad,
                         uint32_t cap, void *stream) {
    const SamWs w = sam_ws_ptrs(ws, B.E);
    return launch_grid(k_sam_ext_items, dim3(sam_grid(B.E, 256, cap)), dim3(256), 0, stream, sam_args(B), w.eread, w.doc, item_seq, item_a, item_row, item_limit, d_bad);
}
// phase 2: the lengths of the extended lines (launch_sam_offsets, k_sam.hip, turns them into offsets)
int launch_sam_ext_len(const SamBatch &B, void *ws, const void *ext, uint32_t cap, void *stream) {
    const SamWs w = sam_ws_ptrs(ws, B.E);
    return launch_grid(k_sam_len_ext, dim3(sam_grid(B.E, 256, cap)), dim3(256), 0, stream, sam_args(B), w.eread, w.doc, static_cast<const SamExtend *>(ext), w.len);
}
// phase 3: the text (total bytes at `text`)
int launch_sam_ext_fill(const SamBatch &B, void *ws, const void *ext, uint64_t total, char *text, uint32_t cap, void *stream) {
    const SamWs w = sam_ws_ptrs(ws, B.E);
    return launch_grid(k_sam_write_ext, dim3(sam_grid(B.E, kSamLines, cap)), dim3(kSamLines), 0, stream, sam_args(B), w.eread, w.doc, w.at, total, text,
                       static_cast<const SamExtend *>(ext));
}

}  // namespace rbg
