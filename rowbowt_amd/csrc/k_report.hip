// k_report.hip -- what rb_markers does with the callback records of the seeding kernels, on the device (rbg_markers_report[_text], include/rbg.h):
//
//   k_read_strands     raw reads -> the 2N-sequence batch: sequence 2i = read i through seq_ntoa_table, 2i + 1 = its reverse complement
//                      (rb_markers.cpp:139-168, :189-198, :396-400)
//   k_seed_canon       per record, in place: the min_range gate, marker_cmp sort, unique, clear_if_conflicting, filter_identical_pos
//   k_seed_canon_big   (:228-236, :266-284, :374-380)
//   k_report_select    per read: which records are printed and in which order (worker :401-413, worker_heuristic :429-519)
//   k_report_len/write the lines, by elements, as k_text.hip writes rb_align's
//
// THE SORT KEY.  MarkerT holds the allele in bits 60-63, the sequence in 48-59 and the position in 0-47; marker_cmp orders by (sequence,
// position, allele), which is the numeric order of rotl64(m, 4) -- a bijection, so sorting on that key and dropping adjacent equals is
// std::sort(marker_cmp) + std::unique.  key >> 4 is (sequence, position).
//
// THE NETWORK.  Every path sorts with the same compare-exchange network, the bitonic sort whose merges start with a "flip" (i against
// i ^ (k - 1)) and go on with i against i ^ j, j = k / 4 ... 1: all exchanges put the smaller key at the lower index, so a segment of any
// length n is sorted by the network of the next power of two with every partner >= n left out (those slots would hold +infinity and never move).
// A group of 4, 16 or 64 lanes holds a segment of at most that many markers in registers and exchanges by cross-lane moves; longer segments
// go on a list and get a workgroup each: 4096-key chunks in LDS, the steps whose distance reaches past a chunk over global memory.
#include <hipcub/hipcub.hpp>

#include "../../include/rbg.h"
#include "rbg_device.hpp"
#include "rbg_text_dev.hpp"

namespace rbg {
namespace {

// ---- strands -----------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint8_t nt_of(const uint8_t b) {   // seq_ntoa_table: ACGT of either case, N/n -> A (sic), anything else -> N
    const uint8_t c = b & 0xDF;
    if (c == 'A' || c == 'C' || c == 'G' || c == 'T') return c;
    return c == 'N' ? 'A' : 'N';
}
__device__ __forceinline__ uint8_t comp_of(const uint8_t c) {   // comp_tab over what nt_of produces
    return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
}

constexpr int kStrandSlot = 48;   // per lane: two aligned 16-byte pieces of the source, one of the output

// One lane makes one aligned 16-byte piece of the output.  The piece is cut where a strand ends; every cut is at most 16 consecutive source
// bytes, fetched as the one or two aligned 16-byte pieces that hold them (neighbouring lanes fetch neighbouring pieces -- ascending on a forward
// strand, descending on a reverse one) and picked apart in the lane's own LDS slot.
__global__ __launch_bounds__(256) void k_read_strands(const uint8_t *__restrict__ seqs, const uint64_t *__restrict__ off, const uint64_t N,
                                                      uint8_t *__restrict__ out, uint64_t *__restrict__ off2) {
    __shared__ __align__(16) uint8_t s_slot[256 * kStrandSlot];
    uint8_t *const slot = s_slot + threadIdx.x * kStrandSlot;
    const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x, stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const uint64_t off0 = off[0], T = off[N] - off0;
    for (uint64_t i = tid; i <= 2 * N; i += stride) {
        const uint64_t r = i >> 1;
        off2[i] = 2 * (off[r] - off0) + ((i & 1) ? off[r + 1] - off[r] : 0);
    }
    const uint64_t nchunks = (2 * T + 15) >> 4;
    for (uint64_t c = tid; c < nchunks; c += stride) {
        uint64_t p = c << 4;
        const uint64_t end = p + 16 < 2 * T ? p + 16 : 2 * T;
        uint64_t lo = 0, hi = N - 1;   // the first read whose two strands end beyond p
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (2 * (off[mid + 1] - off0) > p) hi = mid; else lo = mid + 1;
        }
        uint64_t i = lo;
        *reinterpret_cast<uint4 *>(slot + 32) = make_uint4(0, 0, 0, 0);
        while (p < end) {
            const uint64_t o = off[i], len = off[i + 1] - o, b = 2 * (o - off0);
            if (p >= b + 2 * len) { ++i; continue; }
            const uint64_t r = p - b;
            const bool fwd = r < len;
            const uint64_t u = fwd ? r : r - len;
            const uint64_t n = end - p < len - u ? end - p : len - u;
            const uint64_t a = fwd ? o + u : o + len - u - n;   // source bytes [a, a + n), read upwards (forward) or downwards (reverse)
            const uint64_t a16 = a & ~uint64_t(15);
            *reinterpret_cast<uint4 *>(slot) = *reinterpret_cast<const uint4 *>(seqs + a16);
            if (((a + n - 1) & ~uint64_t(15)) != a16) *reinterpret_cast<uint4 *>(slot + 16) = *reinterpret_cast<const uint4 *>(seqs + a16 + 16);
            const uint32_t s0 = static_cast<uint32_t>(a - a16), d0 = 32 + static_cast<uint32_t>(p & 15), nn = static_cast<uint32_t>(n);
            for (uint32_t j = 0; j < nn; ++j) {
                const uint8_t ch = nt_of(slot[fwd ? s0 + j : s0 + nn - 1 - j]);
                slot[d0 + j] = fwd ? ch : comp_of(ch);
            }
            p += n;
        }
        *reinterpret_cast<uint4 *>(out + (c << 4)) = *reinterpret_cast<const uint4 *>(slot + 32);
    }
}

// ---- canon -------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint64_t mk_key(const uint64_t m) { return (m << 4) | (m >> 60); }
__device__ __forceinline__ uint64_t key_mk(const uint64_t k) { return (k >> 4) | (k << 60); }
constexpr uint64_t kPos48 = (uint64_t(1) << 48) - 1;

struct CanonArgs {
    uint64_t *seeds;     // S records of six u64: lo, hi, qstart, qend, mk_begin, mk_end
    uint64_t S;
    uint64_t *mk;
    uint64_t min_range, read_len;
    uint32_t flags;      // RBG_REPORT_CLEAR_CONFLICTING | RBG_REPORT_CLEAR_IDENTICAL
    uint32_t *big_count, *big_list;   // scratch: header {long segments listed, group width, -, -}, then the list
};

// clear_if_conflicting over the sorted keys' first and last (rb_markers.cpp:279-284)
__device__ __forceinline__ bool keys_conflict(const uint64_t first, const uint64_t last, const uint64_t read_len) {
    return (first >> 52) != (last >> 52) || ((last >> 4) & kPos48) - ((first >> 4) & kPos48) >= read_len;
}
// filter_identical_pos over a sorted, unique list (rb_markers.cpp:266-276): pm starts as marker 0 and only moves to a marker of another (sequence,
// position), markers of one (sequence, position) are neighbours -- so a marker stays iff neither neighbour shares its (sequence, position) and that
// pair is not (0, 0)
__device__ __forceinline__ bool keeps_identical(const uint64_t v, const bool has_prev, const uint64_t pv, const bool has_next, const uint64_t nx) {
    return (v >> 4) != 0 && (!has_prev || (pv >> 4) != (v >> 4)) && (!has_next || (nx >> 4) != (v >> 4));
}

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int G>
__device__ __forceinline__ void canon_groups(const CanonArgs &a, uint64_t *s_slot) {
    const int g = threadIdx.x & (G - 1);
    const uint32_t gshift = (threadIdx.x & 63) & ~(G - 1);
    const uint64_t gmask = G == 64 ? ~uint64_t(0) : (uint64_t(1) << G) - 1;
    uint64_t *const slot = s_slot + (threadIdx.x & ~(G - 1));
    const uint64_t groups = static_cast<uint64_t>(gridDim.x) * blockDim.x / G;
    for (uint64_t s = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / G; s < a.S; s += groups) {
        uint64_t *const rec = a.seeds + 6 * s;
        const uint64_t lo = rec[0], hi = rec[1], b = rec[4], e = rec[5];
        if (e <= b) continue;
        if (hi - lo + 1 < a.min_range) {   // rb_markers.cpp:374: no markers below min_range (wrapping arithmetic, like the reference's)
            if (g == 0) rec[5] = b;
            continue;
        }
        const uint64_t n = e - b;
        if (n > G) {
            if (g == 0) a.big_list[atomicAdd(a.big_count, 1u)] = static_cast<uint32_t>(s);
            continue;
        }
        const int nn = static_cast<int>(n);
        uint64_t k = g < nn ? mk_key(a.mk[b + g]) : 0;
        for (int kk = 2; (kk >> 1) < nn; kk <<= 1) {
            for (int j = kk >> 1, flip = 1; j > 0; j >>= 1, flip = 0) {
                const int partner = flip ? g ^ (kk - 1) : g ^ j;
                const uint64_t other = __shfl(k, partner, G);
                if (g < nn && partner < nn) k = (g < partner) == (k < other) ? k : other;
            }
        }
        const uint64_t first = __shfl(k, 0, G), last = __shfl(k, nn - 1, G), prev = __shfl_up(k, 1, G);
        const bool clear = (a.flags & RBG_REPORT_CLEAR_CONFLICTING) && keys_conflict(first, last, a.read_len);
        const bool keep = g < nn && (g == 0 || k != prev);
        uint64_t m = (__ballot(keep) >> gshift) & gmask;
        uint32_t rank = __popcll(m & ((uint64_t(1) << g) - 1)), cnt = __popcll(m);
        if (!(a.flags & RBG_REPORT_CLEAR_IDENTICAL)) {
            if (keep && !clear) a.mk[b + rank] = key_mk(k);
        } else {
            if (keep) slot[rank] = k;
            wave_lds_fence();
            const bool in = static_cast<uint32_t>(g) < cnt;
            const uint64_t v = in ? slot[g] : 0, pv = in && g > 0 ? slot[g - 1] : 0, nx = static_cast<uint32_t>(g) + 1 < cnt ? slot[g + 1] : 0;
            wave_lds_fence();
            const bool keep2 = in && keeps_identical(v, g > 0, pv, static_cast<uint32_t>(g) + 1 < cnt, nx);
            m = (__ballot(keep2) >> gshift) & gmask;
            rank = __popcll(m & ((uint64_t(1) << g) - 1));
            cnt = __popcll(m);
            if (keep2 && !clear) a.mk[b + rank] = key_mk(v);
        }
        if (g == 0) rec[5] = b + (clear ? 0 : cnt);
    }
}

// the lanes a segment of `mean` markers gets
__device__ __forceinline__ int canon_group_for(const uint64_t total, const uint64_t S) {
    if (total <= 2 * S) return 4;
    if (total <= 8 * S) return 16;
    return 64;
}

// The width is settled BEFORE any record is rewritten (k_seed_canon moves mk_end): one lane leaves it in the scratch header, every wave of
// k_seed_canon reads it from there.  (The markers of a batch lie back to back in record order: the last record's end minus the first one's
// begin is their number; records laid out otherwise get the widest group.)
__global__ void k_seed_canon_width(const CanonArgs a, const int group) {
    a.big_count[0] = 0;
    a.big_count[1] = static_cast<uint32_t>(group ? group : canon_group_for(a.seeds[6 * (a.S - 1) + 5] - a.seeds[4], a.S));
}

__global__ __launch_bounds__(256) void k_seed_canon(const CanonArgs a) {
    __shared__ uint64_t s_slot[256];
    const int G = static_cast<int>(a.big_count[1]);
    if (G == 4) canon_groups<4>(a, s_slot);
    else if (G == 16) canon_groups<16>(a, s_slot);
    else canon_groups<64>(a, s_slot);
}

constexpr uint32_t kCanonChunk = 4096;

// one compare-exchange step over keys [0, n) at `p` (LDS or global): pair q of the step is (i, l), i < l
template <typename Ptr>
__device__ __forceinline__ void cx_step(Ptr p, const uint64_t n, const uint64_t pairs, const uint64_t kk, const uint64_t j, const bool flip) {
    for (uint64_t q = threadIdx.x; q < pairs; q += 256) {
        uint64_t i, l;
        if (flip) {   // (kk is a power of two: block q / (kk / 2) of kk keys, offset q % (kk / 2) in its lower half)
            const uint64_t h = kk >> 1;
            i = ((q & ~(h - 1)) << 1) | (q & (h - 1));
            l = i ^ (kk - 1);
        } else {
            i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
            l = i | j;
        }
        if (l < n) {
            const uint64_t x = p[i], y = p[l];
            if (y < x) { p[i] = y; p[l] = x; }
        }
    }
    __syncthreads();
}
__device__ __forceinline__ uint64_t pow2_at_least(const uint64_t n) {
    uint64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

// unique (IDENT == false) or filter_identical_pos (IDENT == true) over the sorted keys seg[0, n), compacted in place by tiles of 256: a tile's keys
// and their neighbours are read before the tile's survivors are written, and those land at or below where they were read.  Returns the survivors.
template <bool IDENT>
__device__ __forceinline__ uint64_t compact_pass(uint64_t *seg, const uint64_t n) {
    typedef hipcub::BlockScan<uint32_t, 256> Scan;
    __shared__ typename Scan::TempStorage s_scan;
    uint64_t out = 0;
    for (uint64_t t0 = 0; t0 < n; t0 += 256) {
        const uint64_t i = t0 + threadIdx.x;
        const bool in = i < n;
        const uint64_t v = in ? seg[i] : 0, pv = in && i > 0 ? seg[i - 1] : 0, nx = i + 1 < n ? seg[i + 1] : 0;
        const bool keep = in && (IDENT ? keeps_identical(v, i > 0, pv, i + 1 < n, nx) : (i == 0 || v != pv));
        uint32_t rank, total;
        Scan(s_scan).ExclusiveSum(keep ? 1u : 0u, rank, total);
        __syncthreads();
        if (keep) seg[out + rank] = v;
        out += total;
        __syncthreads();
    }
    return out;
}

// one workgroup per listed segment
__global__ __launch_bounds__(256) void k_seed_canon_big(const CanonArgs a) {
    __shared__ uint64_t s_k[kCanonChunk];
    const uint32_t count = *a.big_count;
    for (uint32_t t = blockIdx.x; t < count; t += gridDim.x) {
        uint64_t *const rec = a.seeds + 6 * static_cast<uint64_t>(a.big_list[t]);
        const uint64_t b = rec[4], n = rec[5] - b;
        uint64_t *const seg = a.mk + b;
        // every chunk sorted in LDS (the merges up to the chunk's size never leave it)
        for (uint64_t c0 = 0; c0 < n; c0 += kCanonChunk) {
            const uint64_t m = n - c0 < kCanonChunk ? n - c0 : kCanonChunk;
            for (uint64_t i = threadIdx.x; i < m; i += 256) s_k[i] = mk_key(seg[c0 + i]);
            __syncthreads();
            const uint64_t pairs = pow2_at_least(m) >> 1;
            for (uint64_t kk = 2; (kk >> 1) < m; kk <<= 1) {
                cx_step(s_k, m, pairs, kk, 0, true);
                for (uint64_t j = kk >> 2; j > 0; j >>= 1) cx_step(s_k, m, pairs, kk, j, false);
            }
            for (uint64_t i = threadIdx.x; i < m; i += 256) seg[c0 + i] = s_k[i];
            __syncthreads();
        }
        // the merges across chunks: distances of a chunk and more over global memory, the rest of each merge chunk by chunk in LDS
        if (n > kCanonChunk) {
            const uint64_t pairs = pow2_at_least(n) >> 1;
            for (uint64_t kk = 2 * kCanonChunk; (kk >> 1) < n; kk <<= 1) {
                cx_step(seg, n, pairs, kk, 0, true);
                for (uint64_t j = kk >> 2; j >= kCanonChunk; j >>= 1) cx_step(seg, n, pairs, kk, j, false);
                for (uint64_t c0 = 0; c0 < n; c0 += kCanonChunk) {
                    const uint64_t m = n - c0 < kCanonChunk ? n - c0 : kCanonChunk;
                    for (uint64_t i = threadIdx.x; i < m; i += 256) s_k[i] = seg[c0 + i];
                    __syncthreads();
                    for (uint64_t j = kCanonChunk >> 1; j > 0; j >>= 1) cx_step(s_k, m, kCanonChunk >> 1, kk, j, false);
                    for (uint64_t i = threadIdx.x; i < m; i += 256) seg[c0 + i] = s_k[i];
                    __syncthreads();
                }
            }
        }
        const bool clear = (a.flags & RBG_REPORT_CLEAR_CONFLICTING) && keys_conflict(seg[0], seg[n - 1], a.read_len);
        __syncthreads();
        uint64_t c = compact_pass<false>(seg, n);
        if (!clear && (a.flags & RBG_REPORT_CLEAR_IDENTICAL)) c = compact_pass<true>(seg, c);
        if (clear) c = 0;
        for (uint64_t i = threadIdx.x; i < c; i += 256) seg[i] = key_mk(seg[i]);
        if (threadIdx.x == 0) rec[5] = b + c;
        __syncthreads();
    }
}

// ---- select ------------------------------------------------------------------------------------------------------------------------

struct SelectArgs {
    const uint64_t *seeds;       // canonical records
    const uint64_t *seed_off;    // [2N + 1]: the records of sequence 2i (read i forward) and 2i + 1 (its reverse complement)
    const uint64_t *off2;        // [2N + 1]: the sequences' offsets (their lengths)
    uint64_t N;
    const uint8_t *first_fwd;    // the heuristic worker's coin per read (nullable: forward first)
    uint64_t read_len, min_seed_len;
    uint32_t flags;
};

// the records of read i in print order; FILL: written at out[0 ..), else only counted
template <bool FILL>
__device__ __forceinline__ uint64_t select_read(const SelectArgs &a, const uint64_t i, rbg_report_seed_t *out, uint32_t *out_read) {
    const uint64_t len = a.off2[2 * i + 1] - a.off2[2 * i];
    const bool heuristic = (a.flags & RBG_REPORT_HEURISTIC) != 0, best = heuristic && (a.flags & RBG_REPORT_BEST_STRAND);
    const uint64_t min_len = heuristic ? a.min_seed_len : 0;
    const int first = heuristic && a.first_fwd && !a.first_fwd[i] ? 1 : 0;
    int passes = 2, keep = -1;
    if (best) {   // worker_heuristic's stop rule (:460, looked at between the strands) and keep_seeds_best_strand (:292-314: the first longest seed's strand)
        bool any = false;
        uint64_t best_len = 0;
        for (int pass = 0; pass < passes; ++pass) {
            const int st = pass ? 1 - first : first;
            bool stop = false;
            for (uint64_t s = a.seed_off[2 * i + st]; s < a.seed_off[2 * i + st + 1]; ++s) {
                const uint64_t *rec = a.seeds + 6 * s;
                const uint64_t qlen = rec[3] - rec[2];
                if (rec[1] < rec[0] || qlen < min_len) continue;
                const uint64_t qs = st ? len - rec[2] - 1 : rec[2];
                if (!any || qlen > best_len) { any = true; best_len = qlen; keep = st; }
                if (a.read_len - (qs + qlen) < a.min_seed_len) stop = true;
            }
            if (pass == 0 && stop) passes = 1;
        }
    }
    uint64_t c = 0;
    for (int pass = 0; pass < passes; ++pass) {
        const int st = pass ? 1 - first : first;
        if (keep >= 0 && st != keep) continue;
        for (uint64_t s = a.seed_off[2 * i + st]; s < a.seed_off[2 * i + st + 1]; ++s) {
            const uint64_t *rec = a.seeds + 6 * s;
            const uint64_t qlen = rec[3] - rec[2];
            if (rec[1] < rec[0] || qlen < min_len) continue;   // :373 / :447
            if (FILL) {
                rbg_report_seed_t r;
                r.range_size = rec[1] - rec[0] + 1;
                r.query_start = st ? len - rec[2] - 1 : rec[2];   // :371
                r.query_len = qlen;
                r.mk_begin = rec[4];
                r.mk_end = rec[5] > rec[4] ? rec[5] : rec[4];
                r.strand = static_cast<uint32_t>(st);
                r.pad = 0;
                out[c] = r;
                if (out_read) out_read[c] = static_cast<uint32_t>(i);
            }
            ++c;
        }
    }
    return c;
}

__global__ __launch_bounds__(256) void k_report_select_count(const SelectArgs a, uint64_t *__restrict__ rep_off) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < a.N; i += stride) {
        if (i == 0) rep_off[0] = 0;
        rep_off[i + 1] = select_read<false>(a, i, nullptr, nullptr);
    }
}
__global__ __launch_bounds__(256) void k_report_select(const SelectArgs a, const uint64_t *__restrict__ rep_off, rbg_report_seed_t *__restrict__ out,
                                                       uint32_t *__restrict__ out_read) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < a.N; i += stride)
        (void)select_read<true>(a, i, out + rep_off[i], out_read ? out_read + rep_off[i] : nullptr);
}

// ---- text --------------------------------------------------------------------------------------------------------------------------
// Elements in output order: record r's HEAD ("<name> <range_size> <+|-> <query_start> <query_len>", + " .\n" without markers) is element
// r + melem[r], its markers follow, one element each (" <seq>/<pos>/<allele>"; the last one carries the "\n").

struct RepArgs {
    const rbg_report_seed_t *recs;
    const uint32_t *rec_read;    // the read of every record (its name)
    const uint64_t *melem;       // [R + 1]: exclusive sum of the records' marker counts
    const uint64_t *mk;
    uint64_t R, E;               // records; elements = R + melem[R]
    const char *names;           // the reads' names back to back
    const uint32_t *name_off;    // [reads + 1]
};
__device__ __forceinline__ uint64_t m_seq(const uint64_t m) { return (m >> 48) & 0xFFF; }
__device__ __forceinline__ uint64_t m_pos(const uint64_t m) { return m & kPos48; }
__device__ __forceinline__ uint64_t m_allele(const uint64_t m) { return m >> 60; }

__global__ __launch_bounds__(256) void k_report_mcount(const rbg_report_seed_t *__restrict__ recs, const uint64_t R, uint64_t *__restrict__ melem) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; r < R; r += stride) {
        if (r == 0) melem[0] = 0;
        melem[r + 1] = recs[r].mk_end - recs[r].mk_begin;
    }
}
__global__ __launch_bounds__(256) void k_report_mark(const uint64_t *__restrict__ melem, const uint64_t R, uint32_t *__restrict__ mark) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; r < R; r += stride) mark[r + melem[r]] = static_cast<uint32_t>(r);
}
// the markers of the printed records, dense and in print order (rbg_markers_report's array); the records then point into it
__global__ __launch_bounds__(256) void k_report_gather(const RepArgs a, const uint32_t *__restrict__ erec, rbg_report_seed_t *__restrict__ recs_out,
                                                       uint64_t *__restrict__ dense) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < a.E; e += stride) {
        const uint64_t r = erec[e], h = r + a.melem[r];
        if (e == h) {
            rbg_report_seed_t x = a.recs[r];
            x.mk_begin = a.melem[r];
            x.mk_end = a.melem[r + 1];
            recs_out[r] = x;
        } else {
            dense[e - r - 1] = a.mk[a.recs[r].mk_begin + (e - h - 1)];
        }
    }
}

__global__ __launch_bounds__(256) void k_report_len(const RepArgs a, const uint32_t *__restrict__ erec, uint32_t *__restrict__ len) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < a.E; e += stride) {
        const uint64_t r = erec[e], h = r + a.melem[r], nm = a.melem[r + 1] - a.melem[r];
        if (e == h) {
            const rbg_report_seed_t x = a.recs[r];
            const uint32_t i = a.rec_read[r];
            len[e] = (a.name_off[i + 1] - a.name_off[i]) + 1 + dec_len(x.range_size) + 3 + dec_len(x.query_start) + 1 + dec_len(x.query_len) + (nm ? 0u : 3u);
        } else {
            const uint64_t t = e - h - 1, m = a.mk[a.recs[r].mk_begin + t];
            len[e] = 1 + dec_len(m_seq(m)) + 1 + dec_len(m_pos(m)) + 1 + dec_len(m_allele(m)) + (t + 1 == nm ? 1u : 0u);
        }
    }
}

template <typename Ptr>
__device__ __forceinline__ void put_report_element(const RepArgs &a, const uint64_t e, const uint64_t r, Ptr p) {
    const uint64_t h = r + a.melem[r], nm = a.melem[r + 1] - a.melem[r];
    if (e == h) {
        const rbg_report_seed_t x = a.recs[r];
        const uint32_t i = a.rec_read[r], nb = a.name_off[i], nl = a.name_off[i + 1] - nb;
        for (uint32_t j = 0; j < nl; ++j) p[j] = a.names[nb + j];
        p += nl;
        *p = ' '; p += 1;
        uint32_t n = dec_len(x.range_size);
        put_dec(p, x.range_size, n); p += n;
        p[0] = ' '; p[1] = x.strand ? '-' : '+'; p[2] = ' ';
        p += 3;
        n = dec_len(x.query_start);
        put_dec(p, x.query_start, n); p += n;
        *p = ' '; p += 1;
        n = dec_len(x.query_len);
        put_dec(p, x.query_len, n); p += n;
        if (!nm) { p[0] = ' '; p[1] = '.'; p[2] = '\n'; }
    } else {
        const uint64_t t = e - h - 1, m = a.mk[a.recs[r].mk_begin + t];
        *p = ' '; p += 1;
        uint32_t n = dec_len(m_seq(m));
        put_dec(p, m_seq(m), n); p += n;
        *p = '/'; p += 1;
        n = dec_len(m_pos(m));
        put_dec(p, m_pos(m), n); p += n;
        *p = '/'; p += 1;
        n = dec_len(m_allele(m));
        put_dec(p, m_allele(m), n); p += n;
        if (t + 1 == nm) *p = '\n';
    }
}

constexpr uint32_t kReportLds = 40 * 1024;   // bytes of text a workgroup stages (256 elements of 20-50 bytes; long names take the slow path)

__global__ __launch_bounds__(256) void k_report_write(const RepArgs a, const uint32_t *__restrict__ erec, const uint64_t *__restrict__ at, const uint64_t total,
                                                      char *__restrict__ text) {
    __shared__ __align__(16) char s_buf[kReportLds + 16];
    const uint64_t nblocks = (a.E + 255) / 256;
    for (uint64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const uint64_t e0 = blk * 256, e1 = e0 + 256 < a.E ? e0 + 256 : a.E;
        const uint64_t t0 = at[e0], t1 = e1 < a.E ? at[e1] : total;
        const uint64_t e = e0 + threadIdx.x;
        const uint32_t shift = static_cast<uint32_t>((reinterpret_cast<uintptr_t>(text) + t0) & 15u);   // LDS and memory addresses congruent mod 16
        if (t1 - t0 <= kReportLds) {
            if (e < e1) put_report_element(a, e, erec[e], s_buf + shift + (at[e] - t0));
            __syncthreads();
            const uint32_t nbytes = static_cast<uint32_t>(t1 - t0);
            char *dst = text + t0;
            const char *src = s_buf + shift;
            const uint32_t head = (16u - shift) & 15u;
            const uint32_t h = head < nbytes ? head : nbytes;
            if (threadIdx.x < h) dst[threadIdx.x] = src[threadIdx.x];
            const uint32_t body = (nbytes - h) >> 4;
            for (uint32_t j = threadIdx.x; j < body; j += 256)
                reinterpret_cast<uint4 *>(dst + h)[j] = reinterpret_cast<const uint4 *>(src + h)[j];
            const uint32_t done = h + (body << 4);
            if (threadIdx.x < nbytes - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
            __syncthreads();
        } else if (e < e1) {
            put_report_element(a, e, erec[e], text + at[e]);   // (long names: straight to memory)
        }
    }
}

struct MaxOp {
    __device__ __forceinline__ uint32_t operator()(uint32_t x, uint32_t y) const { return x > y ? x : y; }
};

inline int grid_for(const uint64_t n) { return static_cast<int>(std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), 256ull * 32)); }
inline size_t up256(const size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace

// ---- launchers (all asynchronous on `stream`; hipError_t as int) ---------------------------------------------------------------------

// total: any upper bound on off[N] - off[0] (it sizes the grid); out: 16-byte aligned, ((2 * total + 15) & ~15) bytes at least; off2[2N + 1]
int launch_read_strands(const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t total, uint8_t *out, uint64_t *off2, void *stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (N == 0) return static_cast<int>(hipMemsetAsync(off2, 0, 8, st));
    hipLaunchKernelGGL(k_read_strands, dim3(grid_for(std::max<uint64_t>((2 * total + 15) / 16, 2 * N + 1))), dim3(256), 0, st, seqs, off, N, out, off2);
    return static_cast<int>(hipGetLastError());
}

int report_canon_group() {
    const char *e = std::getenv("RBG_REPORT_GROUP");
    const int v = e ? std::atoi(e) : 0;
    return v == 4 || v == 16 || v == 64 ? v : 0;
}
size_t seed_canon_tmp_bytes(uint64_t S) { return 16 + 4 * static_cast<size_t>(S); }

int launch_seed_canon(const LaunchCfg &cfg, uint64_t *seeds, uint64_t S, uint64_t *mk, uint64_t min_range, uint32_t flags, uint64_t read_len, void *tmp,
                      size_t tmp_bytes, int group, void *stream) {
    if (S == 0) return 0;
    if (tmp_bytes < seed_canon_tmp_bytes(S) || (S >> 32) || (reinterpret_cast<uintptr_t>(tmp) & 3)) return static_cast<int>(hipErrorInvalidValue);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const CanonArgs a{seeds, S, mk, min_range, read_len, flags, static_cast<uint32_t *>(tmp), static_cast<uint32_t *>(tmp) + 4};
    const uint64_t w = group ? static_cast<uint64_t>(group) : 64u;   // the grid for the widest group: a narrower one finds more groups in the same threads
    int blocks = static_cast<int>(std::min<uint64_t>((S * w + 255) / 256, 256ull * 32));
    if (cfg.max_blocks > 0) blocks = std::min(blocks, cfg.max_blocks);
    hipLaunchKernelGGL(k_seed_canon_width, dim3(1), dim3(1), 0, st, a, group);
    hipLaunchKernelGGL(k_seed_canon, dim3(std::max(blocks, 1)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_seed_canon_big, dim3(static_cast<int>(std::min<uint64_t>(S, 1024))), dim3(256), 0, st, a);
    return static_cast<int>(hipGetLastError());
}

int launch_report_select(const uint64_t *seeds, const uint64_t *seed_off, const uint64_t *off2, uint64_t N, const uint8_t *first_fwd, uint64_t read_len,
                         uint64_t min_seed_len, uint32_t flags, uint64_t *rep_off, void *out, uint32_t *out_read, void *tmp, size_t tmp_bytes,
                         void *stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (N == 0) return static_cast<int>(hipMemsetAsync(rep_off, 0, 8, st));
    const SelectArgs a{seeds, seed_off, off2, N, first_fwd, read_len, min_seed_len, flags};
    hipLaunchKernelGGL(k_report_select_count, dim3(grid_for(N)), dim3(256), 0, st, a, rep_off);
    const int e = scan_in_place(rep_off + 1, N, tmp, tmp_bytes, st);   // (the caller's scratch: aligned and checked against the scan's need there)
    if (e) return e;
    hipLaunchKernelGGL(k_report_select, dim3(grid_for(N)), dim3(256), 0, st, a, rep_off, static_cast<rbg_report_seed_t *>(out), out_read);
    return static_cast<int>(hipGetLastError());
}

// melem[R + 1] = exclusive sum of the records' marker counts (tmp: scan_tmp_bytes(R))
int launch_report_melem(const void *recs, uint64_t R, uint64_t *melem, void *tmp, size_t tmp_bytes, void *stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (R == 0) return static_cast<int>(hipMemsetAsync(melem, 0, 8, st));
    hipLaunchKernelGGL(k_report_mcount, dim3(grid_for(R)), dim3(256), 0, st, static_cast<const rbg_report_seed_t *>(recs), R, melem);
    const int e = scan_in_place(melem + 1, R, tmp, tmp_bytes, st);   // (the caller's scratch, as above)
    return e ? e : static_cast<int>(hipGetLastError());
}

// workspace of E elements: erec / len (4 bytes each), at (8), the scans' temporaries
size_t report_text_ws_bytes(uint64_t E) {
    size_t s1 = 0, s2 = 0;
    (void)hipcub::DeviceScan::InclusiveScan(nullptr, s1, static_cast<uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr), MaxOp(), static_cast<int64_t>(E ? E : 1));
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, s2, static_cast<uint32_t *>(nullptr), static_cast<uint64_t *>(nullptr), static_cast<int64_t>(E ? E : 1));
    return 2 * up256(E * 4) + up256(E * 8 + 8) + up256(std::max(s1, s2)) + 1024;
}
namespace {
struct RepWs {
    uint32_t *erec, *len;
    uint64_t *at;
    void *tmp;
    size_t tmp_bytes;
};
RepWs rep_ws(void *ws, size_t ws_bytes, uint64_t E) {
    char *b = static_cast<char *>(ws);
    const size_t fixed = 2 * up256(E * 4) + up256(E * 8 + 8);
    return RepWs{reinterpret_cast<uint32_t *>(b), reinterpret_cast<uint32_t *>(b + up256(E * 4)), reinterpret_cast<uint64_t *>(b + 2 * up256(E * 4)), b + fixed,
                 ws_bytes - fixed};
}
}  // namespace

// every element's record (E = R + melem[R] >= 1, R < 2^32)
int launch_report_map(const uint64_t *melem, uint64_t R, uint64_t E, void *ws, size_t ws_bytes, void *stream) {
    if (ws_bytes < report_text_ws_bytes(E) || (reinterpret_cast<uintptr_t>(ws) & 255) || (R >> 32)) return static_cast<int>(hipErrorInvalidValue);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RepWs w = rep_ws(ws, ws_bytes, E);
    hipError_t e = hipMemsetAsync(w.erec, 0, E * 4, st);
    if (e != hipSuccess) return static_cast<int>(e);
    hipLaunchKernelGGL(k_report_mark, dim3(grid_for(R)), dim3(256), 0, st, melem, R, w.erec);
    size_t tb = w.tmp_bytes;
    e = hipcub::DeviceScan::InclusiveScan(w.tmp, tb, w.erec, w.erec, MaxOp(), static_cast<int64_t>(E), st);
    return static_cast<int>(e != hipSuccess ? e : hipGetLastError());
}
const uint32_t *report_map_erec(const void *ws) { return static_cast<const uint32_t *>(ws); }   // (rep_ws: the map comes first)
int launch_report_gather(const void *recs, const uint64_t *melem, const uint64_t *mk, uint64_t R, uint64_t E, void *ws, size_t ws_bytes, void *recs_out,
                         uint64_t *dense, void *stream) {
    const RepWs w = rep_ws(ws, ws_bytes, E);
    const RepArgs a{static_cast<const rbg_report_seed_t *>(recs), nullptr, melem, mk, R, E, nullptr, nullptr};
    hipLaunchKernelGGL(k_report_gather, dim3(grid_for(E)), dim3(256), 0, static_cast<hipStream_t>(stream), a, w.erec, static_cast<rbg_report_seed_t *>(recs_out), dense);
    return static_cast<int>(hipGetLastError());
}
// lengths and offsets of the elements; the text has at[E - 1] + len[E - 1] bytes (report_text_total_ptrs)
int launch_report_text_plan(const void *recs, const uint32_t *rec_read, const uint64_t *melem, const uint64_t *mk, uint64_t R, uint64_t E, const char *names,
                            const uint32_t *name_off, void *ws, size_t ws_bytes, void *stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RepWs w = rep_ws(ws, ws_bytes, E);
    const RepArgs a{static_cast<const rbg_report_seed_t *>(recs), rec_read, melem, mk, R, E, names, name_off};
    hipLaunchKernelGGL(k_report_len, dim3(grid_for(E)), dim3(256), 0, st, a, w.erec, w.len);
    size_t tb = w.tmp_bytes;
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum(w.tmp, tb, w.len, w.at, static_cast<int64_t>(E), st);
    return static_cast<int>(e != hipSuccess ? e : hipGetLastError());
}
void report_text_total_ptrs(void *ws, uint64_t E, const uint64_t **last_at, const uint32_t **last_len) {
    const RepWs w = rep_ws(ws, 0, E);
    *last_len = w.len + (E - 1);
    *last_at = w.at + (E - 1);
}
int launch_report_text_fill(const void *recs, const uint32_t *rec_read, const uint64_t *melem, const uint64_t *mk, uint64_t R, uint64_t E, const char *names,
                            const uint32_t *name_off, void *ws, size_t ws_bytes, uint64_t total, char *text, void *stream) {
    const RepWs w = rep_ws(ws, ws_bytes, E);
    const RepArgs a{static_cast<const rbg_report_seed_t *>(recs), rec_read, melem, mk, R, E, names, name_off};
    hipLaunchKernelGGL(k_report_write, dim3(static_cast<int>(std::min<uint64_t>((E + 255) / 256, 256ull * 16))), dim3(256), 0, static_cast<hipStream_t>(stream), a,
                       w.erec, w.at, total, text);
    return static_cast<int>(hipGetLastError());
}

}  // namespace rbg
