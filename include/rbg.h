/*
 * rbg.h -- C-ABI of the MI355X-native backward-search engine for rowbowt's rb_align hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Everything the
 * reference computes on this path through rbwt::RowBowt<ri::rle_string_sd> is reachable here,
 * batched over N reads.  Each entry point cites the reference interface it replaces
 * (paths relative to the reference tree).  The C++17 header shim that keeps the reference's own
 * signatures on top of this ABI is rowbowt_amd/include/rowbowt_gpu.hpp; the binding a reference
 * maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *  - Ranges are inclusive [lo,hi]; the empty range is exactly {1,0} (rowbowt.hpp:77,85).
 *  - All positions are uint64_t.  Reads are raw bytes, matched as-is (no upper-casing, no N
 *    handling: rb_align.cpp:121 passes seq->seq.s straight to find_range).
 *  - A batch of reads is `seqs` (concatenated bytes) + `off[N+1]` (byte offsets, off[0]=0).
 *  - Return value: RBG_OK (0) or a negative RBG_E* code; rbg_strerror() names it.  The reference
 *    itself prints to stderr and exit(1)s (rowbowt_io.hpp:166-169); the shim maps codes to that.
 *  - There is NO CPU compute path.  Every query entry point runs HIP kernels on a gfx950 device
 *    and fails with RBG_ENODEV when none is usable.
 *  - *_dev entry points take DEVICE pointers and a hipStream_t (as void*), launch asynchronously
 *    and neither allocate nor synchronise (graph-capturable).  The plain entry points take HOST
 *    pointers, stage through HBM and block until the results are in the caller's buffers.
 *  - Thread safety: an rbg_index is immutable after load; concurrent query calls on one index
 *    are allowed (the reference calls const methods concurrently, rb_markers.cpp:321-326).
 */
#ifndef RBG_H
#define RBG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 3 (round 5): RBG_OPT_KMER_STEPS goes up to 8 (default 8: the run-indexed layout steps by up to eight symbols; the slot layout by
 * up to five); rbg_info_t ends with depth_runs[8]; rbg_layout_info_t holds eight depths and lost the fields of the retired first format;
 * the options RBG_OPT_TREE_TOP_KB (12), RBG_OPT_SLOT_BYTES (13) and RBG_OPT_RUN_FMT (15) are gone (RBG_EARG) together with the kernels they
 * selected.  ABI 2 -> 3 also records what round 4 changed without a bump: the default HBM budget is a
 * quarter of the free HBM (was three quarters), RBG_LAYOUT_AUTO builds the run-indexed layout when the slot tables of every symbol per step
 * do not fit it, rbg_layout_info / rbg_sample_reads_pangenome_dev / RBG_LAYOUT_PREFER_SLOTS / options 16-17 exist.  A binding should check
 * rbg_abi_version() before it binds the symbols of a newer ABI (rowbowt_amd/capi.py does). */
#define RBG_ABI_VERSION 3

typedef struct rbg_index rbg_index;

/* rbwt::LoadRbwtFlag, rowbowt_io.hpp:146-152 (same values) */
enum { RBG_LOAD_NONE = 0, RBG_LOAD_SA = 1, RBG_LOAD_MA = 2, RBG_LOAD_DL = 4, RBG_LOAD_FT = 8 };

enum {
    RBG_OK = 0,
    RBG_EIO = -1,      /* file missing / unreadable (reference: "bad file", exit(1)) */
    RBG_EFORMAT = -2,  /* not the sdsl layout the reference's files use */
    RBG_ENODEV = -3,   /* no usable gfx950 device / HIP error */
    RBG_EARG = -4,     /* bad argument */
    RBG_ENOMEM = -5,
    RBG_ENOTLOADED = -6 /* structure (toehold SA / markers / docs) was not loaded */
};

/* device = HIP device ordinal to hold the index replica, or RBG_DEVICE_NONE to parse and flatten
 * on the host only (no queries possible; used to inspect the layout without a GPU). */
#define RBG_DEVICE_NONE (-1)

int rbg_abi_version(void);
const char *rbg_strerror(int code);

/* ---- loading ------------------------------------------------------------------------------ */

/* rbwt::load_rowbowt<ri::rle_string_sd>(prefix, flag), rowbowt_io.hpp:176-189:
 * reads <prefix>.rbwt always, .tsa if SA, .mab if MA, .docs if DL (suffixes :17-21) in the
 * sdsl-serialised layout the reference writes (rle_string.hpp:248-275, toehold_sa.hpp:74-91),
 * flattens to the HBM layout and uploads one replica to `device`.
 * RBG_LOAD_FT is accepted and ignored (rb_align never sets it, rb_align.cpp:149-157). */
int rbg_load(const char *prefix, int flags, int device, rbg_index **out);

/* Construction from raw inputs, replacing rle_string(std::string fname, B) rle_string.hpp:44-97
 * and ToeholdSA(n, r, ssa, esa) toehold_sa.hpp:27-35 at run granularity:
 * heads[R]/lens[R] = run-length BWT (byte 0 must already be stored as 1, rle_string.hpp:59,62);
 * ssa_y/esa_y = the second u64 of each (x,y) pair of <pre>.ssa / <pre>.esa, one per BWT run
 * (toehold_sa.hpp:133-155), or both NULL for no toehold SA. */
int rbg_build_from_runs(const uint8_t *heads, const uint64_t *lens, uint64_t R,
                        const uint64_t *ssa_y, const uint64_t *esa_y, int device, rbg_index **out);

/* Next-row f1: the same construction straight from rb_build's raw input files (rb_build.cpp:83-93):
 * <pre>.bwt read as rle_string(fname) reads it (formatted extraction skips whitespace bytes,
 * rle_string.hpp:58-62; byte 0 -> 1), <pre>.ssa / <pre>.esa as (x,y) u64 pairs (both or neither). */
int rbg_build_from_files(const char *bwt_fname, const char *ssa_fname, const char *esa_fname, int device,
                         rbg_index **out);

/* ---- next-row f1: native cache file and the rb_build outputs ----------------------------------
 * "<prefix>.rbgpu" holds what the reference's .rbwt/.tsa/.mab/.docs hold, as flat little-endian
 * arrays with a checksum (layout: rowbowt_amd/csrc/rbg_host.hpp; the file is mapped and checked by all loader threads:
 * 1.2 s for the 9 GB of an n = 5e10 index); loading it needs no sdsl decoding.
 * rbg_load() falls back to "<prefix>.rbgpu" when "<prefix>.rbwt" does not exist.
 * rbg_convert_index: the reference's serialised files (rb_build's output, rowbowt_io.hpp:49-89) -> cache.
 * rbg_convert_raw:   rb_build's raw inputs <pre>.bwt [+ .ssa/.esa] (rb_build.cpp:83-93; rle_string.hpp:44-97,
 *                    toehold_sa.hpp:27-35,133-155), plus optionally an already serialised .mab and a
 *                    .docs file -> cache.  (The raw .ma input is read by pfbwt-f's MarkerArray
 *                    constructor, which is not vendored: not supported.)
 * Both run on the host only.  rbg_load_cache: flags select the stored parts; asking for a part the
 * file lacks is RBG_EIO, like a missing .tsa/.mab/.docs. */
int rbg_convert_index(const char *prefix, int flags, const char *out_path);
int rbg_convert_raw(const char *bwt_fname, const char *ssa_fname, const char *esa_fname, const char *mab_fname,
                    const char *docs_fname, const char *out_path);
int rbg_load_cache(const char *path, int flags, int device, rbg_index **out);
/* the cache file from a run-length BWT in memory (the arguments of rbg_build_from_runs): for builders that never write
 * the BWT as text, and for handing one index to the ranks of a node (rank 0 writes, every rank rbg_load_cache's) */
int rbg_convert_runs(const uint8_t *heads, const uint64_t *lens, uint64_t R, const uint64_t *ssa_y /* nullable, with esa_y */,
                     const uint64_t *esa_y, const char *out_path);
/* the same with a marker array (the arguments of rbg_set_markers; mk_nruns = 0: none) and the text of a .docs file
 * (nullable) stored beside it: one file that rb_align -s -m / rb_markers can run from */
int rbg_convert_runs_markers(const uint8_t *heads, const uint64_t *lens, uint64_t R, const uint64_t *ssa_y, const uint64_t *esa_y,
                             const uint64_t *mk_start, const uint64_t *mk_end, uint64_t mk_nruns, const uint64_t *mk_off,
                             const uint64_t *mk_vals, const char *docs_text /* nullable */, const char *out_path);
/* RowBowt::build_ftab(k) + FTab::serialize (rowbowt.hpp:726-744, ftab.hpp:29-34): the reference's
 * text .ftab ("<kmer> <lo> <hi>" per line, lexicographic), computed with the search kernel. 1 <= k <= 16. */
int rbg_write_ftab(rbg_index *, uint64_t k, const char *path);
/* What loading a .ftab amounts to here (LoadRbwtFlag::FT, rowbowt_io.hpp:187; FTab::load, ftab.hpp:15-27):
 * the file must be, byte for byte, the table build_ftab(k) makes for this index (RBG_EFORMAT if not);
 * *k_out = its k-mer size, the `ftab_k` argument of the marker-seed calls below. */
int rbg_check_ftab(rbg_index *, const char *path, uint64_t *k_out);
/* MarkerArray contents (pfbwt-f marker_array.hpp, loaded at rowbowt_io.hpp:185):
 * inclusive SA-index runs + mk_off[nruns+1] offsets into mk_vals. */
int rbg_set_markers(rbg_index *, const uint64_t *run_start, const uint64_t *run_end, uint64_t nruns,
                    const uint64_t *mk_off, const uint64_t *mk_vals);
/* A SECOND marker table, keyed by TEXT position (the reference's rle_window_arr `midx`, rb_markers_tsa.cpp:76-101: rb_locs looks up the markers
 * that overlap the text interval a read aligns to).  Arguments as rbg_set_markers; the runs are inclusive, ascending, disjoint intervals of text
 * positions in [0, n) (anything else: RBG_EARG).  It lives beside the SA-row table and never replaces it; setting it again replaces the table
 * set before (whose device memory is given back).  On the primary only (RBG_EARG on a replica): rbg_replicate* carries the table a primary has
 * at that moment.  Needs a device (RBG_ENODEV on a host-only handle). */
int rbg_set_text_markers(rbg_index *, const uint64_t *run_start, const uint64_t *run_end, uint64_t nruns,
                         const uint64_t *mk_off, const uint64_t *mk_vals);
/* the same from a <prefix>.midx file, read with the .mab reader.  That the two files share a format is INFERRED, not pinned: rle_window_arr and
 * MarkerArray come from the same pfbwt-f header family (not vendored with the reference), and build_midx.cpp and rowbowt_io.hpp:60 construct and
 * serialise them the same way (three sd_vectors -- run starts, run ends, first-value flags -- then the int_vector of values); no file written
 * by the reference's build_midx was available to check against.  RBG_EIO / RBG_EFORMAT as for the other index files. */
int rbg_load_text_markers(rbg_index *, const char *path);
/* DocList contents, doclist.hpp:57-73: names '\0'-joined, starts[ndocs].  A second call replaces the table (and frees the device copy of the first one's
 * sorted starts): rbg_set_docs must not overlap queries on the handle. */
int rbg_set_docs(rbg_index *, const char *names_joined, const uint64_t *starts, uint64_t ndocs);

void rbg_free(rbg_index *);

/* ---- introspection ------------------------------------------------------------------------ */

typedef struct rbg_info_t {
    uint64_t n;             /* rle_string::size() */
    uint64_t r;             /* rle_string::number_of_runs() */
    uint32_t sigma;         /* distinct BWT symbols */
    uint32_t pos_bytes;     /* 4 or 8: width of positions in the HBM layout */
    int32_t device;         /* HIP ordinal or RBG_DEVICE_NONE */
    uint32_t has_tsa, has_markers, has_docs;
    uint64_t hbm_bytes;     /* bytes of the device replica */
    uint64_t marker_runs, marker_vals;
    uint32_t rank_bucket_shift, phi_bucket_shift;
    uint32_t slot_bytes;    /* bytes per rank slot of the slot layout: 16; 0 on the run-indexed layout or without a device */
    /* first-level slot tables: totals and how many buckets overflow their 2 inline entries */
    uint64_t rank_slots, rank_slots_overflow, phi_slots, phi_slots_overflow;
    /* multi-symbol LF steps: symbols consumed per gather (1..5), size of the major alphabet that has
     * k-mer tables (0 = none), total runs of the 2-mer and 3-mer tables */
    uint64_t kmer_steps, kmer_symbols, pair_runs, triple_runs, quad_runs;
    /* ftab (RowBowt::build_ftab / search_ftab, rowbowt.hpp:726-758): word length of the device table, 0 = none */
    uint64_t ftab_k;
    uint64_t quint_runs;    /* total runs of the 5-mer tables (kmer_steps == 5) */
    /* ABI 2: how the space/speed point was chosen at load (the same call is up to 4x slower with fewer levels,
     * DESIGN.md 2b): the depth asked for (RBG_OPT_KMER_STEPS), the free HBM seen at load, the budget the replica had
     * to fit (a quarter of it, or RBG_OPT_HBM_BUDGET_MB); kmer_steps above is what was kept.  Also printed on
     * stderr at load when a level is dropped (always with RBG_VERBOSE). */
    uint64_t kmer_steps_requested, hbm_free_at_load, hbm_budget;
    uint64_t rank_layout;   /* RBG_LAYOUT_SLOTS or RBG_LAYOUT_RUNS (what RBG_OPT_RANK_LAYOUT / the budget rule chose) */
    uint64_t replicas;      /* per handle: 1 when this handle holds a device replica, 0 for a host-only index
                             * (RBG_DEVICE_NONE); further replicas are handles of their own (rbg_replicate[_many]) */
    uint64_t depth_runs[8]; /* ABI 3: [d - 1] = total runs of the tables of k-mer depth d ([0] = r; 0 for a depth that has no tables,
                             * or no run lists on the run-indexed layout); pair_runs .. quint_runs above are [1] .. [4] */
} rbg_info_t;
enum { RBG_LAYOUT_AUTO = 0, RBG_LAYOUT_SLOTS = 1, RBG_LAYOUT_RUNS = 2, RBG_LAYOUT_PREFER_SLOTS = 3 };
int rbg_info(const rbg_index *, rbg_info_t *out);   /* writes sizeof(rbg_info_t) bytes of THIS header: a client built against another ABI uses ... */
int rbg_info_sized(const rbg_index *, rbg_info_t *out, uint64_t out_bytes);   /* ... this: min(out_bytes, sizeof) bytes; fields are only added at the end from ABI 3 on */

/* What the load decided about the run-indexed layout (RBG_LAYOUT_RUNS), so that no table is left out silently: the
 * reference's structures have no size limits (rle_string.hpp:131-161, toehold_sa.hpp:56-72 are plain uint64_t), and where
 * this layout has one -- or the HBM budget bites -- the decision is here and on stderr.  All zero on the slot layout.
 * out_bytes = sizeof(rbg_layout_info_t) of the caller (fields beyond it are not written: the struct may grow at its end). */
typedef struct rbg_layout_info_t {
    uint32_t run_fmt;                 /* 2 (the per-lane search; the wave-cooperative format 1 of rounds 2-3 was retired in round 5) */
    uint32_t depths_composed;         /* k-mer depths the load composed run lists for (1..8) */
    uint32_t depth_mask_asked;        /* RBG_OPT_RUN_DEPTHS as given (0 = the default rule) */
    uint32_t depth_mask_kept;         /* bit d - 1: depth d has run lists in HBM */
    uint32_t depths_dropped_budget;   /* bit d - 1: depth d was left out because the replica exceeded the HBM budget */
    uint32_t rank_directories;        /* 1: some depth's ranks go through per-table directories (a depth with bucket records has rec_bytes > 0) */
    uint32_t phi_directory;           /* 1: phi goes through its directory */
    uint32_t fill_shift;              /* 8-byte positions: entries of a table lie less than 2^fill_shift rows apart */
    uint64_t entries[8];              /* per depth: entries of its run lists (sentinels and fillers included) */
    uint64_t fillers[8];              /* per depth: filler entries among them (8-byte positions; 0 unless a table has a gap >= 2^fill_shift) */
    uint64_t dir_bytes[8];            /* per depth: bytes of its tables' directories */
    uint64_t phi_entries, phi_fillers, phi_dir_bytes, phi_dir_shift;
    uint64_t phi_slots, phi_slot_bytes; /* phi SLOTS (RBG_OPT_RUN_PHI): their number (buckets of 2^phi_dir_shift text positions) and the
                                         * bytes of slots + ordinals; 0 = phi goes through the list of sampled positions and its directory */
    uint64_t rec_bytes[8];            /* per depth: bytes of its tables' bucket records (RBG_OPT_RUN_REC; 0 = directories) */
    uint64_t rec_overflow[8];         /* per depth: buckets with more entries than a record holds (their ranks go through the run list) */
    uint64_t budget_raised;           /* 1: RBG_LAYOUT_AUTO, no budget given, took three quarters of the free HBM instead of a quarter -- an index of so many runs
                                       * that the quarter would have left it one or two symbols per step (rbg_info().hbm_budget is the budget applied) */
} rbg_layout_info_t;
int rbg_layout_info(const rbg_index *, rbg_layout_info_t *out, uint64_t out_bytes);

/* The jump table (RBG_OPT_JUMP_K): for every K-mer that OCCURS in the text, the search state after it, so that a read of
 * at least K symbols replaces its first K backward-search steps by one probe.  The reference's ftab (RowBowt::search_ftab,
 * rowbowt.hpp:121-131, :726-758) made sparse; result-neutral.  Built last at load (rbg_load, rbg_load_cache, rbg_build_*), from what
 * the HBM budget leaves after every other decision -- the layout is the one the load makes without it -- and copied by rbg_replicate;
 * not stored in a cache file.  4-byte positions and the run-indexed layout only.  All zero when no table was built (RBG_VERBOSE=1
 * says why). */
typedef struct rbg_jump_info_t {
    uint64_t k;          /* symbols per key */
    uint64_t keys;       /* K-mers in the table */
    uint64_t bytes;      /* HBM of the table (counted in rbg_info().hbm_bytes) */
    uint64_t buckets;    /* 64-byte buckets of two slots */
    double build_ms;     /* wall time of enumerating, searching and inserting the keys */
    /* Level 2 (RBG_OPT_JUMP2_K), a second table probed after a hit of the first: the state after every occurring word of k + k2 symbols,
     * keyed by the k2 symbols and the first table's lo.  Only rbg_jump_info_sized fills these; all zero when there is none. */
    uint64_t k2;         /* symbols per key of level 2 */
    uint64_t keys2;
    uint64_t bytes2;     /* (counted in rbg_info().hbm_bytes as well) */
    uint64_t buckets2;
    double build2_ms;    /* wall time of level 2 alone; build_ms does not include it */
    /* The levels that are complete: bit 0 = level 1, bit 1 = level 2.  Every word that occurs in the text is in a complete table, so a read whose
     * key it lacks has an empty range and ends at the probe instead of walking the ftab path to the same answer.  A level whose build left a word
     * out is not complete; RBG_JUMP_ABSENT_ENDS=0 in the environment of a load leaves none (same tables, same answers).  Only rbg_jump_info_sized
     * with a buffer of at least 88 bytes fills it. */
    uint64_t complete;
} rbg_jump_info_t;
int rbg_jump_info(const rbg_index *, rbg_jump_info_t *out);   /* the first five fields (40 bytes), as before level 2 existed */
int rbg_jump_info_sized(const rbg_index *, rbg_jump_info_t *out, uint64_t out_bytes);   /* min(out_bytes, sizeof) bytes; fields are only added at the end */

/* RowBowt::get_f(), rowbowt.hpp:719 / build_f :770-778: 256 entries. */
int rbg_get_f(const rbg_index *, uint64_t f_out[256]);
/* ToeholdSA::get_last_run_sample(), toehold_sa.hpp:97-99 */
int rbg_last_run_sample(const rbg_index *, uint64_t *out);

/* Host copies of the flattened layout, for layout tests (no compute).  Each call returns the
 * element count in *count and, if dst != NULL, copies min(*count, cap) uint64 values.
 * which: */
enum {
    RBG_ARR_RUN_HEADS = 0,   /* R values (head byte of each BWT run) */
    RBG_ARR_RUN_START = 1,   /* R+1 values (BWT position where each run starts; last = n) */
    RBG_ARR_SAMPLES_LAST = 2,/* r values: ToeholdSA::samples_last_ (toehold_sa.hpp:158) */
    RBG_ARR_PRED_POS = 3,    /* r values: set bits of ToeholdSA::pred_ (:157) */
    RBG_ARR_PHI_BASE = 4,    /* r values: samples_last_[pred_to_run_[j]-1] (:70), 0 where run 0 */
    RBG_ARR_MARKER_START = 5, RBG_ARR_MARKER_END = 6, RBG_ARR_MARKER_OFF = 7, RBG_ARR_MARKER_VALS = 8
};
int rbg_host_array(const rbg_index *, int which, uint64_t *dst, uint64_t cap, uint64_t *count);

/* ---- queries, host buffers (drop-in) ------------------------------------------------------ */

/* RowBowt::LF(range_t, uint8_t c), rowbowt.hpp:74-88: one backward step for N (range, symbol)
 * triples.  An input range outside [0,n) x [0,n) or an absent symbol yields {1,0}. */
int rbg_lf(rbg_index *, const uint64_t *lo, const uint64_t *hi, const uint8_t *sym, uint64_t N,
           uint64_t *lo_out, uint64_t *hi_out);
/* RowBowt::find_range(const std::string&), rowbowt.hpp:121-131, for N reads. */
int rbg_find_range(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N,
                   uint64_t *lo, uint64_t *hi);
/* RowBowt::count, rowbowt.hpp:266-269. */
int rbg_count(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t *count);
/* find_range (ssamp == NULL) / find_range_w_toehold for reads that lie scattered in a larger host buffer: read i =
 * base[begin[i], begin[i] + len[i]).  What a FASTA/FASTQ parser that leaves the sequence bytes in its input buffer
 * hands over (the reference copies every read into a std::string first, rb_align.cpp:97): no gather on the host. */
int rbg_find_range_spans(rbg_index *, const uint8_t *base, const uint64_t *begin, const uint32_t *len, uint64_t N,
                         uint64_t *lo, uint64_t *hi, uint64_t *ssamp /* nullable */);

/* RowBowt::find_range_w_toehold, rowbowt.hpp:169-184 (LFData.rn / .ssamp); a failed read gets
 * {1,0}, ssamp=0 (LFData::clear :153-159).  RBG_ENOTLOADED without a toehold SA. */
int rbg_find_range_w_toehold(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N,
                             uint64_t *lo, uint64_t *hi, uint64_t *ssamp);
/* RowBowt::locs_at(range, k, max_hits, locs), rowbowt.hpp:613-615 -> ToeholdSA::locate_range
 * toehold_sa.hpp:37-49, for N (range, toehold) triples.  loc_off[N+1] is written (exclusive scan
 * of min(occ,max_hits)); *locs is malloc()ed by the library with loc_off[N] entries and must be
 * released with rbg_free_buffer.  Per read the order is SA[hi], SA[hi-1], ... (phi chain). */
int rbg_locs_at(rbg_index *, const uint64_t *lo, const uint64_t *hi, const uint64_t *k, uint64_t N,
                uint64_t max_hits, uint64_t *loc_off, uint64_t **locs);
/* RowBowt::markers_at(range_t, vec), rowbowt.hpp:282-285 -> MarkerArray::at_range. */
int rbg_markers_at(rbg_index *, const uint64_t *lo, const uint64_t *hi, uint64_t N,
                   uint64_t *mk_off, uint64_t **mk);
/* RowBowt::find_range_w_markers(query, wsize, max_range), rowbowt.hpp:292-339: final range plus
 * the windowed marker list (window results PREPENDED, :320,:333). */
int rbg_find_range_w_markers(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N,
                             uint64_t wsize, uint64_t max_range,
                             uint64_t *lo, uint64_t *hi, uint64_t *mk_off, uint64_t **mk);
/* Next-row f4 (marker seeds).  RowBowt::get_markers_greedy_seeding(query, wsize, max_range, fn),
 * rowbowt.hpp:406-482, as rb_markers runs it (rb_markers.cpp:411-413): one record per call of the
 * callback fn(range, (q.first, q.second), mbuf), in call order.  ftab_k = 0: no ftab loaded
 * (rb_markers' default, rb_markers.cpp:25); ftab_k = K > 0: with the ftab of k-mer size K loaded
 * (rb_markers --ftab): the first K bases and every restart after a failed seed go through
 * search_ftab (rowbowt.hpp:430-433, :454-464), computed as find_range of the ACGT-only k-mer (see
 * rbg_check_ftab).  A read shorter than K makes the reference throw (substr, :431); here its
 * first lookup counts as a miss.  The reference requires K - 1 <= wsize (:423-426).  The
 * markers are NOT sorted or deduplicated (the caller's out_fn does that, rb_markers.cpp:374-380).
 * Works without a marker array too (every mbuf empty), like the reference (:273, :283). */
typedef struct rbg_marker_seed {
    uint64_t lo, hi;     /* range passed to fn (never empty in this variant) */
    uint64_t qstart;     /* q.first */
    uint64_t qend;       /* q.second + 1 (exclusive end; q.second itself wraps for an empty seed) */
    uint64_t mk_begin;   /* this seed's mbuf = mk[mk_begin, mk_end) */
    uint64_t mk_end;
} rbg_marker_seed_t;
/* seed_off[N+1] written; *seeds (seed_off[N] records) and *mk are malloc()ed by the library:
 * release both with rbg_free_buffer. */
int rbg_get_markers_greedy_seeding(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N,
                                   uint64_t wsize, uint64_t max_range, uint64_t ftab_k,
                                   uint64_t *seed_off, rbg_marker_seed_t **seeds, uint64_t **mk);
/* RowBowt::get_markers_lmems(query, wsize, max_range, fn), rowbowt.hpp:341-404 (rb_markers --ftab --lmem): a fresh backward
 * search from every end position e = m, m-1, ..., 1 of each sequence, in callback order; the same records and arguments as
 * rbg_get_markers_greedy_seeding.  Only the non-empty calls are returned -- exactly len(sequence) records per sequence, so
 * seed_off[] == off[] -- the reference's second call after a failed extension (the empty range, the same q, an empty mbuf)
 * is left to the caller (rowbowt_gpu.hpp replays it; rb_markers drops it).  ftab_k = 0: plain longest matches from the full
 * range; ftab_k = K > 0: as with the ftab of k-mer size K loaded (the check "ftab must be enabled!" and K - 1 <= wsize are the
 * caller's, as in the reference, :346-354).  Quirks kept:
 *   1. search_ftab answers a miss (an absent K-mer, or any byte outside ACGT) with the FULL range (:746-758), so :371-373 is
 *      never taken: the walk goes on from the full range with K symbols counted, and the record includes them.
 *   2. the ftab part does not move the window end: the first window query comes after the first step past the K-mer.
 *   3. a suffix shorter than K starts from the full range without the ftab (no substr past the end, unlike the greedy mode).
 *   4. a failure at the first symbol (e.g. an N at e - 1) reports the full range with length 0 (qstart = qend = e).
 * Markers are unsorted and not deduplicated, as in the greedy call.  The batch is walked on the device in passes of about
 * 4 Mi records (RBG_LMEM_CHUNK), so device memory stays bounded; the host result is 48 bytes per symbol. */
int rbg_get_markers_lmems(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N,
                          uint64_t wsize, uint64_t max_range, uint64_t ftab_k,
                          uint64_t *seed_off, rbg_marker_seed_t **seeds, uint64_t **mk);
/* Next-row f4 (greedy seeding).  RowBowt::get_seeds_greedy_w_sample(query, min_length),
 * rowbowt.hpp:222-256, reduced by the choice locate_from_longest_seed makes (rowbowt.hpp:669-677):
 * per read the FIRST seed of strictly greatest length, as LFData {rn, qstart, qend, ssamp}; a read
 * with no seed of at least min_length gets rn={1,0}, qstart=qend=ssamp=0. */
int rbg_greedy_longest_seed(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t min_length,
                            uint64_t *lo, uint64_t *hi, uint64_t *qstart, uint64_t *qend, uint64_t *ssamp);
/* The whole seed list of RowBowt::get_seeds_greedy_w_sample(query, min_length) (rowbowt.hpp:222-256; flags = RBG_SEEDS_W_SAMPLE) or
 * RowBowt::get_seeds_greedy(query, min_length, lfdata) (:191-215; flags = 0): every greedy seed of every read as LFData {rn, qstart,
 * qend, ssamp}, where rbg_greedy_longest_seed keeps one.  seed_off[N+1]: read i owns records [seed_off[i], seed_off[i+1]), in the
 * reference's order (the first record is the rightmost seed).  *seeds is ONE block of 5 * seed_off[N] u64, five arrays back to back:
 * lo | hi | qstart | qend | ssamp (release with rbg_free_buffer) -- arrays and not records, because lo / hi / ssamp are what
 * rbg_locate_plan_dev / rbg_locate_order_dev take and qstart is the d_sub of rbg_locate_fill_offset_dev (locate_from_longest_seed's
 * "minus qstart", :684-686).  Quirks kept:
 *   1. with the sample the last record (qstart = 0) is pushed only if ei >= min_length (:252); without it, always, whatever its
 *      length (:211).
 *   2. without the sample the reference leaves ssamp uninitialised (LFData's three-argument constructor, :148-152, :163): here it is
 *      0.  flags = 0 works on an index loaded without a toehold SA.
 *   3. with the sample and no toehold SA every list is empty (:225) -- RBG_OK, not RBG_ENOTLOADED.
 *   4. pk is not reset when a seed fails (:241-244): a zero-length seed (recorded only when min_length == 0, e.g. at the second of
 *      two N) carries the toehold of the last successful step anywhere earlier in that read, or 2^64 - 1 if there was none; its
 *      range is the full range.
 *   5. an empty read gives one record {full range, 0, 0, 2^64 - 1} when min_length == 0 (without the sample: always, ssamp 0), and
 *      no record otherwise.
 *   6. any byte that does not occur in the BWT (N, lower case) ends a seed and is skipped. */
#define RBG_SEEDS_W_SAMPLE 1u
int rbg_get_seeds_greedy(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t min_length, uint32_t flags,
                         uint64_t *seed_off, uint64_t **seeds);
/* RowBowt::find_range_w_toehold_chkpnts(query, wsize), rowbowt.hpp:575-606: one backward search per read with a record {rn, qstart,
 * qend, ssamp} after step i = wsize, 2 wsize, ... <= m - 1 (step i consumes q[m-i-1]; the test of :592).  Such a record is labelled
 * qstart = m - i, qend = the previous label (m at first), but its range and toehold are those of q[m-i-1, m): one symbol more than
 * the label says -- {rn, ssamp} of a record with qstart = s > 0 is rbg_find_range_w_toehold(q[s-1:]).  A final record {qstart 0,
 * qend m} with the whole read's range follows when (m - 1) % wsize != 0.  A read that occurs therefore has floor((m - 1) / wsize)
 * records, plus one if (m - 1) % wsize != 0 (m >= 1; a one-symbol read has none); a read that does not occur has none (:588-590).
 * An empty read: no step, m - 1 wraps -- one record {full range, 0, 0, last run sample} if (2^64 - 1) % wsize != 0, none otherwise
 * (wsize 1, 3, 5, 15, 17, ...).  wsize == 0 is RBG_EARG (the reference computes % 0).  Without a toehold SA every list is empty
 * (:579).  Output as rbg_get_seeds_greedy: seed_off[N+1] and one block of 5 * seed_off[N] u64 (lo | hi | qstart | qend | ssamp). */
int rbg_find_range_w_toehold_chkpnts(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t wsize,
                                     uint64_t *seed_off, uint64_t **seeds);
/* RowBowt::find_locs_greedy_seeding(s, min_length, max_hits), rowbowt.hpp:633-657 (== get_seeds +
 * locate_from_longest_seed :664-685): locations of the longest seed, each minus the seed's qstart. */
int rbg_find_locs_greedy_seeding(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t min_length,
                                 uint64_t max_hits, uint64_t *loc_off, uint64_t **locs);
/* The markers of the text-position table (rbg_set_text_markers) over the text intervals of located reads: read i has the locations
 * locs[loc_off[i], loc_off[i+1]) (as rbg_find_locs_greedy_seeding / rbg_locs_at return them) and the length off[i+1] - off[i]; for a location
 * l its interval is [l, l + m - 1] in wrapping 64-bit arithmetic -- empty when the end lies below the start (m == 0; a location that wrapped
 * below zero whose end wraps back) or when l >= n; an end beyond the text is clamped to n - 1.  mk_off[N+1] is per READ: *mk holds read i's
 * markers for its first location, then its second, ...; within a location in run order -- the order rb_markers_tsa.cpp:80-86 prints.
 * RBG_ENOTLOADED without a text-position table. */
int rbg_markers_at_locs(rbg_index *, const uint64_t *locs, const uint64_t *loc_off, const uint64_t *off, uint64_t N,
                        uint64_t *mk_off, uint64_t **mk);
/* one read of rb_locs, batched (rb_markers_tsa.cpp:76-88): rbg_find_locs_greedy_seeding, then rbg_markers_at_locs over its result, the
 * locations staying on the device in between.  *locs and *mk through rbg_free_buffer. */
int rbg_find_loc_markers_greedy_seeding(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t min_length,
                                        uint64_t max_hits, uint64_t *loc_off, uint64_t **locs, uint64_t *mk_off, uint64_t **mk);
/* gives back a result array one of the calls above allocated (*locs, *mk, *seeds).  Always through this call, never free():
 * large blocks are kept and handed to the next result of about that size -- their pages are already there, which is most of
 * what a 3 GB result costs (RBG_RESULT_POOL=0 in the environment: plain malloc / free). */
void rbg_free_buffer(void *);

/* RowBowt::resolve_offset, rowbowt.hpp:623-625 -> DocList::doc_and_offset_at doclist.hpp:46-50.
 * *name points into the index (valid until rbg_free). */
int rbg_resolve_offset(const rbg_index *, uint64_t i, const char **name, uint64_t *offset);
/* The table rbg_resolve_offset answers from, for callers that resolve positions by the million: position i belongs to
 * document names[k - 1] at offset i - sorted_starts[k - 1], k = # sorted_starts < min(i + 1, size) (doclist.hpp:46-50,
 * :77-79; k == 0 has no answer: rbg_resolve_offset returns RBG_EARG there).  Pointers stay valid until rbg_free. */
int rbg_doc_table(rbg_index *, uint64_t *ndocs, const uint64_t **sorted_starts, const char *const **names, uint64_t *size);

/* `rb_align -s` as text, made on the device (rb_report, rb_align.cpp:118-139): for every read
 *     <name> (<lo>,<hi>), count=<hi - lo + 1>\n\tlocs: <pos>/<doc>:<pos - doc start> ... \n
 * with locs_at (rowbowt.hpp:613-621, max_hits as in rbg_locs_at) and resolve_offset (:623-625, doclist.hpp:46-79) done
 * where the ranges are: the locations never cross PCIe, the decimals are written by kernels, the host gets the finished
 * bytes.  lo / hi / k: host arrays of N (from rbg_find_range_w_toehold / rbg_find_range_spans); the names are N spans of
 * name_base (name_begin[i], name_len[i]).  *text points into a pinned buffer the handle owns: valid until
 * rbg_release_text(ix, *text) (several may be out at once: a writer thread can still hold one while the next batch is
 * made).  The call returns while the text is still being copied out (on the handle's own copy stream, under the caller's
 * next calls): rbg_wait_text(ix, *text) before the first byte is read.  RBG_ENOTLOADED without the toehold SA or the document list; RBG_EARG when a location lies before every
 * document (rbg_resolve_offset's error).  k == NULL: the report without -s, one line per read (no toehold SA or
 * document list needed). */
enum { RBG_TEXT_MARKERS = 1 };   /* flags: also "\tmarkers: <pos>/<allele> ...\n" per read (markers_at, rb_align.cpp:134-142; needs the marker array) */
int rbg_align_text(rbg_index *, const uint64_t *lo, const uint64_t *hi, const uint64_t *k, uint64_t N, uint64_t max_hits, uint32_t flags,
                   const char *name_base, const uint64_t *name_begin, const uint32_t *name_len, const char **text, uint64_t *text_len);
int rbg_wait_text(rbg_index *, const char *text);
int rbg_release_text(rbg_index *, const char *text);
/* make `count` pinned text buffers of `bytes` now (pinning a few hundred MB takes tenths of a second: a tool does it before its clock starts) */
int rbg_reserve_text(rbg_index *, uint64_t bytes, int count);
/* ---- SAM lines of raw reads, both strands, written on the device ------------------------------------------------------------------------
 * Per read: the greedy seeds (rbg_greedy_longest_seed's choice, min_length >= 1) of the read as given and of its reverse complement -- ACGTacgt ->
 * TGCAtgca, every other byte itself, so an N stays N and ends a seed (not rb_markers' seq_ntoa_table) --; the strand with the longer seed is kept, a tie
 * goes to forward; its locations in locate order (locs_at with the seed's toehold) are resolved as rbg_resolve_offset resolves them.  With the read's
 * length m and the seed [a, b) in the searched orientation, tab-separated and "\n"-terminated:
 *   mapped, primary (location 1, SA[hi])   QNAME FLAG RNAME POS 255 CIGAR * 0 0 SEQ QUAL NH:i:<hi - lo + 1> HI:i:1
 *       FLAG 16 on the reverse strand, else 0; POS = the offset of the seed's own text position in its document + 1 (nothing is subtracted for the
 *       a clipped bases); CIGAR = [a "S"] (b - a) "M" [(m - b) "S"]; SEQ the searched orientation, QUAL reversed with it ("*" without qual_base)
 *   secondary (RBG_SAM_SECONDARY only), locations j = 2 .. min(occ, max_hits):  the same with FLAG | 256, SEQ "*", QUAL "*", HI:i:<j>
 *   unmapped (no seed of min_length on either strand)   QNAME 4 * 0 0 * * 0 0 SEQ QUAL   the read as given, no tags; an empty read: SEQ "*", QUAL "*"
 * Without RBG_SAM_SECONDARY max_hits is taken as 1 for the walk (and max_hits == 0 as 1 with it: the primary line is always there).  MAPQ is always 255.
 * The document of a line is that of its first aligned base: a seed that runs over a document boundary is NOT detected.
 * Reads, qualities (qual_base nullable: every QUAL is "*"; read i's quality is the seq_len[i] bytes at qual_begin[i]) and names are N spans of their
 * bases.  *text is one of the handle's pinned text buffers with rbg_align_text's protocol (rbg_wait_text, rbg_release_text, rbg_reserve_text); N == 0
 * gives *text = NULL, *text_len = 0.  RBG_ENOTLOADED without the toehold SA or the document list; RBG_EARG: min_length == 0 (a zero-length seed has
 * the full range), unknown flags, N >= 2^32, 2^32 or more bytes of reads or of names, a location before every document (as rbg_align_text).  Works
 * on replicas.  rbg_counters: reads += 2N (both strands searched), locations += every location walked, once.  RBG_SAM_TRACE=1 prints the steps' times at
 * exit; RBG_SAM_GRID_CAP=<workgroups> caps the grids of the call's own kernels (tests, A/Bs). */
#define RBG_SAM_SECONDARY 1u   /* also one line per further location, up to max_hits */
int rbg_align_sam(rbg_index *, const char *seq_base, const uint64_t *seq_begin, const uint32_t *seq_len,
                  const char *qual_base /* nullable: every QUAL is "*" */, const uint64_t *qual_begin /* lengths = seq_len */,
                  const char *name_base, const uint64_t *name_begin, const uint32_t *name_len, uint64_t N,
                  uint64_t min_length, uint64_t max_hits, uint32_t flags, const char **text, uint64_t *text_len);
/* ---- the same lines with every seed extended LEFTWARDS through mismatches, by an LF walk ------------------------------------------------------
 * rbg_align_sam's steps through the locate fill, then per LINE (each location of a read by itself: two haplotypes that share the seed may differ in the
 * flank and get different NM and MD): the row of the line's occurrence is known -- line j of the range [lo, hi] is row hi - (j - 1) --, BWT[row] is the
 * reference base left of it and LF(row) the row of the occurrence one base further left, so the left flank is read base by base from the index and compared
 * with the read's clipped prefix.  With s the searched orientation, [a, b) the seed, offs the location's offset in its document and K = max_mismatch:
 *     L = min(a, offs)                       never leaves the read, never crosses the document's start
 *     score = best = 0; e = 0; nm = 0; mm = 0; r = row
 *     for t in 0 .. L-1:
 *         c = BWT[r]                         one of the bytes A C G T, else stop (terminator, separator, N, anything else)
 *         x = s[a-1-t]                       bytes compared as they are: a lower-case or N read base is a mismatch
 *         if c == x: score += 1
 *         else: mm += 1; if mm > K: stop     the (K+1)-th mismatch is not taken
 *               score -= 4; remember (t, c)
 *         if score >= best: best = score; e = t + 1; nm = mm
 *         r = LF(r, c)
 * e is the extension (it ends on a match; trailing mismatches fall away), nm the mismatches inside it, AS = (b - a) + best.  A mapped line differs from
 * rbg_align_sam's in POS = offs + 1 - e, CIGAR = [(a-e)S] (b-a+e)M [(m-b)S] and three tags after HI: NM:i:<nm>, MD:Z:<match counts separated by the
 * reference base of each mismatch, over the read positions [a-e, b); it starts and ends with a number>, AS:i:<AS> -- on every mapped line, also at e = 0.
 * Unmapped lines, FLAG, RNAME, SEQ, QUAL, NH, HI and the strand pick (the longer seed) are rbg_align_sam's.  THERE IS NO RIGHT EXTENSION: LF only goes
 * left and the index holds no FL structure; the right flank stays soft-clipped.  Arguments, text-buffer protocol, errors and counters as rbg_align_sam;
 * RBG_EARG also for max_mismatch > RBG_SAM_MAX_MISMATCH and for a NULL handle.  Works on replicas.  RBG_SAM_TRACE=1 prints this call's steps on a line of its own, with an
 * `extend` column (items + walks); RBG_SAM_GRID_CAP caps its grids too. */
#define RBG_SAM_MAX_MISMATCH 8
int rbg_align_sam_extend(rbg_index *, const char *seq_base, const uint64_t *seq_begin, const uint32_t *seq_len,
                         const char *qual_base /* nullable: every QUAL is "*" */, const uint64_t *qual_begin /* lengths = seq_len */,
                         const char *name_base, const uint64_t *name_begin, const uint32_t *name_len, uint64_t N,
                         uint64_t min_length, uint64_t max_hits, uint32_t flags, uint32_t max_mismatch, const char **text, uint64_t *text_len);
/* The walk alone, one lane per item: item j extends leftwards from position d_item_a[j] of sequence d_item_seq[j] of the batch (d_seqs 16-byte aligned,
 * d_off[N + 1], as the *_dev searches take it), whose base at a lies at row d_item_row[j] of the suffix array's order; it goes at most d_item_limit[j]
 * bases (offs).  d_out[j]: ext = e, nm, score = best, steps = the bases taken (LF steps), and EVERY taken mismatch in the order met -- mis_t[k] = its t,
 * mis_ref[k] = the reference base; the first nm of them lie inside the extension, unused entries are zero.  RBG_EARG for max_mismatch >
 * RBG_SAM_MAX_MISMATCH (before anything runs).  The items are checked on the device -- a sequence index >= N, an a beyond its sequence, a row >= n: the
 * item's record is zero, the others are walked -- and reported when the kernel has run: this call WAITS for `stream` and then returns RBG_EARG.  Works on
 * replicas. */
typedef struct rbg_extend_t {
    uint32_t ext, nm;
    int32_t score;
    uint32_t steps;
    uint32_t mis_t[8];
    uint8_t mis_ref[8];
} rbg_extend_t;
int rbg_extend_left_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, const uint32_t *d_item_seq /* [M] */,
                        const uint32_t *d_item_a /* [M] */, const uint64_t *d_item_row /* [M] */, const uint64_t *d_item_limit /* [M]: offs */, uint64_t M,
                        uint32_t max_mismatch, rbg_extend_t *d_out /* [M] */, void *stream);
/* ---- the FL index, and the same lines extended on BOTH sides -----------------------------------------------------------------------------------
 * FL(i) = select_c(BWT, i - F[c]) is the inverse of LF: from the row of the suffix at text position p it gives T[p] -- the row's F symbol c -- and the row of
 * the suffix at p + 1.  rbg_fl_prepare builds it from the handle's run heads and run starts and uploads it to THIS handle's device (rbg_fl.hpp): per base of
 * A C G T the c-runs of the BWT in BWT order as {symbols of c before the run, BWT position of its start} (2 x 4 bytes at 4-byte positions, else 2 x 8) with a
 * closing sentinel, and a directory over rank, dir[k >> shift] = the run that holds rank (k >> shift) << shift, shift = max(0, floor(log2(n_c / runs_c))), of
 * (n_c >> shift) + 2 entries of the position width.  Its bytes: the sum over the bases present of (runs_c + 1) * 2 * pos_bytes + ((n_c >> shift) + 2) *
 * pos_bytes -- proportional to r.  Opt-in: no load builds it.  Idempotent; the allocation counts in rbg_info's hbm_bytes.  Per handle: a replica prepares
 * its own copy (from its root's host arrays).  RBG_ENOTLOADED when the host run arrays are not there.  It must not overlap queries on the handle.
 * rbg_fl_info: out[0] = prepared (0 / 1), out[1] = the structure's bytes on the device (the formula above), out[2 .. 5] = the runs of A C G T, out[6] =
 * their shifts, 8 bits each (A in the lowest), out[7] = the directory entries of all four.  Every *_dev call below and rbg_align_sam_extend_both answer
 * RBG_ENOTLOADED until the handle has been prepared. */
int rbg_fl_prepare(rbg_index *);
int rbg_fl_info(const rbg_index *, uint64_t out[8]);
/* FL of M rows, one lane per row: d_sym[j] = the F byte of row d_rows[j] when it is one of A C G T, else 0 (terminator, separator, N, anything else);
 * d_next[j] = FL(row), 2^64 - 1 when there is no base.  A row >= n gives sym 0 and next 0 and is reported when the kernel has run: the call WAITS for `stream`
 * and returns RBG_EARG (the other rows are answered).  RBG_SAM_GRID_CAP caps the grid. */
int rbg_fl_dev(rbg_index *, const uint64_t *d_rows, uint64_t M, uint8_t *d_sym, uint64_t *d_next, void *stream);
/* The right walk alone, one lane per item: item j extends rightwards from position d_item_b[j] (the seed's end) of sequence d_item_seq[j] of the batch (d_seqs
 * 16-byte aligned, d_off[N + 1]); d_item_row[j] is the row of the suffix at which the walk starts and d_item_skip[j] the FL steps it first takes without comparing
 * -- from the row of the seed's first base, skip = b - a crosses the seed; a row without a base on the way ends the item with a zero record (no error).  Then,
 * with s the sequence, m its length and K = max_mismatch:
 *     L = min(m - b, limit); score = best = 0; e = 0; nm = 0; mm = 0
 *     for t in 0 .. L-1:
 *         c = the F symbol of r                one of the bytes A C G T, else stop
 *         x = s[b + t]                         bytes compared as they are
 *         if c == x: score += 1
 *         else: mm += 1; if mm > K: stop; score -= 4; remember (t, c)
 *         if score >= best: best = score; e = t + 1; nm = mm
 *         r = FL(r)
 * d_out[j] as rbg_extend_left_dev's record with t counted rightwards from b; `steps` counts the compared bases only.  Item errors (the record is zero, the
 * others are walked, RBG_EARG after the kernel has run): a sequence index >= N, a b beyond its sequence, skip > b, a row >= n.  Works on prepared replicas. */
int rbg_extend_right_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, const uint32_t *d_item_seq /* [M] */,
                         const uint32_t *d_item_b /* [M] */, const uint64_t *d_item_row /* [M] */, const uint32_t *d_item_skip /* [M] */,
                         const uint64_t *d_item_limit /* [M] */, uint64_t M, uint32_t max_mismatch, rbg_extend_t *d_out /* [M] */, void *stream);
/* rbg_align_sam_extend through its left walk, unchanged, then per LINE that has a right clip (m > b; other lines make no item and cost no walk) the right walk
 * above with row = the line's own row, skip = b - a, limit = doc_end - (location + (b - a)) -- doc_end the next sorted document start, n for the last
 * document -- and the budget K - nmL, so a line's NM never exceeds max_mismatch.  The line: POS as rbg_align_sam_extend gives it, CIGAR = [(a-eL)S]
 * (b-a+eL+eR)M [(m-b-eR)S], NM = nmL + nmR, MD over the read positions [a-eL, b+eR) (left part, seed, right part), AS = (b-a) + bestL + bestR.  A line
 * without a right clip is rbg_align_sam_extend's line.  Unchanged: the strand pick (the longer SEED, not the longer alignment), and a seed that spans a
 * document boundary stays undetected (nothing is walked right of it).  Arguments, text-buffer protocol, errors and counters as rbg_align_sam_extend;
 * RBG_ENOTLOADED without rbg_fl_prepare on this handle.  RBG_SAM_TRACE=1 prints a line of its own with an `extend right` column and the walks' sums. */
int rbg_align_sam_extend_both(rbg_index *, const char *seq_base, const uint64_t *seq_begin, const uint32_t *seq_len,
                              const char *qual_base /* nullable */, const uint64_t *qual_begin, const char *name_base, const uint64_t *name_begin,
                              const uint32_t *name_len, uint64_t N, uint64_t min_length, uint64_t max_hits, uint32_t flags, uint32_t max_mismatch,
                              const char **text, uint64_t *text_len);
/* The header that goes with those lines (host): "@HD\tVN:1.6\tSO:unsorted\n", then per document in sorted-start order "@SQ\tSN:<name>\tLN:<len>\n", then
 * pg_line as given (nullable).  len = the next sorted start - this one, for the last document rbg_info().n - its start: an UPPER BOUND of the
 * sequence's length, which includes the separators between documents and the terminator.  *text: NUL-terminated, through rbg_free_buffer.
 * RBG_ENOTLOADED without a document list. */
int rbg_sam_header(rbg_index *, const char *pg_line /* nullable, appended as given */, char **text, uint64_t *text_len);
/* ---- extract: the indexed text read back from the index -----------------------------------------------------------------------------------------
 * The ISA sample (rbg_isa.hpp) maps a text position to the row of its suffix.  rbg_extract_prepare runs rbg_fl_prepare if needed, then builds the sample from
 * the handle's host arrays and uploads it to THIS handle's device: pairs {tpos, row}, tpos = SA[row], of (1) the last row of every BWT run (the toehold's
 * run-end samples) and (2) every row whose BWT symbol is not one of A C G T and that does not end its run (its SA by the host's phi rule from the run's last
 * row downwards) -- the second group puts a sample right behind every non-base byte of the text, so no non-base byte lies between a position and the sample
 * before it, and position 0 is always a sample.  Sorted by tpos, S entries of 2 x pos_bytes, with a directory over text position, dir[b] = the largest sample
 * with tpos <= b << shift, shift = max(0, floor(log2(n / S))), (n >> shift) + 2 entries of the position width.  Its bytes: S * 2 * pos_bytes + ((n >> shift)
 * + 2) * pos_bytes.  The row of p is p - q FL steps from the row of the sample {q, row_q} with the largest q <= p.  Opt-in: no load builds it, no load rule or
 * budget changes.  Idempotent; one allocation, counted in rbg_info's hbm_bytes.  Per handle: a replica prepares its own copy (from its root's host arrays).
 * RBG_ENOTLOADED when the handle has no toehold samples or no run arrays.  It must not overlap queries on the handle.
 * rbg_extract_info: out[0] = prepared (0 / 1), out[1] = the sample's bytes on the device (the formula above), out[2] = S, out[3] = shift, out[4] = the
 * directory's entries, out[5] = the samples of the second kind, out[6] = the largest gap between neighbouring samples (n closing the list): a walk-in takes
 * fewer FL steps than that, out[7] = the build and upload time in microseconds.  Every call below answers RBG_ENOTLOADED until the handle has been prepared,
 * and RBG_OK for M == 0 after that. */
int rbg_extract_prepare(rbg_index *);
int rbg_extract_info(const rbg_index *, uint64_t out[8]);
/* The rows of M text positions, one lane per position: d_row[j] = the row of the suffix at d_pos[j] (ISA).  A position >= n gives row 0 and is reported
 * when the kernel has run: the call WAITS for `stream` and returns RBG_EARG (the other positions are answered).  RBG_SAM_GRID_CAP caps the grid. */
int rbg_isa_dev(rbg_index *, const uint64_t *d_pos, uint64_t M, uint64_t *d_row, void *stream);
/* the same from host memory (RBG_EARG for a position >= n: nothing is written) */
int rbg_isa(rbg_index *, const uint64_t *pos, uint64_t M, uint64_t *row);
/* The text of M intervals, one lane per item: item j writes EXACTLY d_len[j] bytes at d_out + d_out_off[j] -- the bytes of the text from d_pos[j] on up to the
 * first one that is not a base of A C G T (a separator, an N, the terminator), d_got[j] of them, then zeros.  An interval that would run past n ends at the
 * terminator by that rule: no error.  A position >= n writes zeros, got 0, and is reported when the kernel has run: the call WAITS for `stream` and returns
 * RBG_EARG (the other items are answered).  The items' stretches of d_out must not overlap; nothing else of d_out is touched.  One lane walks one item, so a
 * long interval is best given as many items (rbg_extract does that).  RBG_SAM_GRID_CAP caps the grid. */
int rbg_extract_dev(rbg_index *, const uint64_t *d_pos, const uint32_t *d_len, const uint64_t *d_out_off, uint64_t M, uint8_t *d_out /* bytes */,
                    uint32_t *d_got /* [M] */, void *stream);
/* The same from host memory: `out` is the concatenation of the intervals in item order (interval j at the exclusive sum of len[0 .. j)), got[j] the bases of
 * interval j, zeros behind them.  Every interval is cut into pieces of at most RBG_OPT_EXTRACT_CHUNK bases before the upload, each an item that finds its
 * own row; the interval ends at its first short piece, so the result does not depend on the chunk.  RBG_EARG for a pos[j] >= n (nothing is written). */
int rbg_extract(rbg_index *, const uint64_t *pos, const uint64_t *len, uint64_t M, uint8_t *out, uint64_t *got);
/* ---- an index from its text: suffix array, runs, samples (sa_build.hip) ---------------------------------------------------------------
 * The text is n bytes whose LAST byte is its unique smallest one (the terminator; rb_build --fasta writes documents joined by '#' and ends in 0x01).  The
 * three device calls take no handle and run on the current device, like rbg_sample_reads_dev.  pos_bytes = 4 (n < 2^32 - 16 only) or 8 (any n): the width
 * of ranks and of suffix-array entries.
 * rbg_suffix_array_dev: d_sa[i] = the start of the i-th smallest suffix, n entries of pos_bytes; exactly n * pos_bytes bytes are written at d_sa (aligned to
 * pos_bytes) and nothing outside d_sa and d_tmp (rbg_sa_tmp_bytes(n, pos_bytes) bytes, 256-byte aligned; 0 = a width that does not hold n).  Prefix
 * doubling over ranks from a first key of eight bytes; suffixes whose rank is unique leave the later rounds.  The rule about the last byte is checked on the
 * device before anything is sorted: RBG_EARG, d_sa untouched.  RBG_EARG also for n == 0, a NULL or misaligned pointer, too little scratch.  NOT
 * capturable: the call waits for `stream` once per round and has finished when it returns.
 * rbg_sa_info: of the last rbg_suffix_array_dev / rbg_build_from_text / rbg_convert_text of the process -- out[0] = rounds (the first key's round included;
 * at most ceil(log2 n) + 1), out[1] = the elements sorted, summed over the rounds (at most n * rounds), out[2] = the scratch bytes, out[3] = n, out[4] =
 * pos_bytes, out[5] = the suffixes still tied after the first round, out[6 .. 7] = 0.
 * rbg_text_runs_plan_dev: *R = the runs of the BWT, BWT[i] = text[(SA[i] - 1) mod n] with byte 0 read as 1 (rle_string.hpp:59,62); the runs are numbered in
 * d_tmp (rbg_text_runs_tmp_bytes, 256-byte aligned).  Waits for `stream`.  rbg_text_runs_fill_dev, with the same d_tmp: d_heads[R] (u8), d_lens[R], d_ssa[R],
 * d_esa[R] (u64) -- the arguments of rbg_build_from_runs: the raw SA values at each run's first and last row (toehold_sa.hpp:133-155).  Asynchronous.
 * Both read d_sa as n entries of pos_bytes, aligned to pos_bytes.  R is the plan's count; with a smaller R (>= 1) the call returns 0, writes the first R
 * runs in full and nothing behind entry R - 1 of any array.  RBG_EARG, nothing written: n == 0, R == 0 or R > n, a NULL or misaligned pointer (d_tmp,
 * d_sa), too little scratch, a pos_bytes that is not 4 or 8 or does not hold n. */
size_t rbg_sa_tmp_bytes(uint64_t n, uint32_t pos_bytes);
int rbg_suffix_array_dev(const uint8_t *d_text, uint64_t n, void *d_sa, uint32_t pos_bytes, void *d_tmp, size_t tmp_bytes, void *stream);
int rbg_sa_info(uint64_t out[8]);
size_t rbg_text_runs_tmp_bytes(uint64_t n, uint32_t pos_bytes);
int rbg_text_runs_plan_dev(const uint8_t *d_text, const void *d_sa, uint64_t n, uint32_t pos_bytes, void *d_tmp, size_t tmp_bytes, uint64_t *R, void *stream);
int rbg_text_runs_fill_dev(const uint8_t *d_text, const void *d_sa, uint64_t n, uint32_t pos_bytes, const void *d_tmp, size_t tmp_bytes, uint64_t R,
                           uint8_t *d_heads, uint64_t *d_lens, uint64_t *d_ssa, uint64_t *d_esa, void *stream);
/* The same from a text in HOST memory, to a handle: upload, the three calls above, then rbg_build_from_runs' own path (with RBG_LOAD_SA in flags the toehold
 * samples are kept, without it none; other flag bits are ignored).  The position width follows RBG_OPT_POS_BYTES.  Before anything is allocated the device
 * bytes of the build -- n + n * pos_bytes + max(rbg_sa_tmp_bytes, rbg_text_runs_tmp_bytes) -- are compared with hipMemGetInfo's free bytes: RBG_ENOMEM when
 * they do not fit (the text is not touched).  The run arrays, 25 bytes per run, are checked the same way once the plan has counted the runs: RBG_ENOMEM
 * again, before any of the four is allocated.  RBG_ENODEV for device = RBG_DEVICE_NONE, RBG_EARG for n == 0, a NULL text, a text that breaks the rule.
 * rbg_convert_text: the cache file instead of a handle, through rbg_convert_runs_markers (docs_text nullable, as there). */
int rbg_build_from_text(const uint8_t *text, uint64_t n, int flags, int device, rbg_index **out);
int rbg_convert_text(const uint8_t *text, uint64_t n, const char *docs_text /* nullable */, int flags, int device, const char *out_path);
/* ---- the marker array from variant sites, over the suffix array (mk_build.hip) --------------------------------------------------------
 * A SITE RECORD is (pos, first, val): pos = the text position of a variant site in one haplotype copy; first = the first text position of its window,
 * max(start of pos's document, pos - w + 1); val = the MarkerT (allele index in bits 60-63, contig index in bits 48-59, 0-based reference position in the
 * low 48 bits).  The S records are strictly ascending in pos; first does not descend, first <= pos < n and pos - first < w (1 <= w <= 64).
 *   - the row i with p = SA[i] carries the values of every record with first <= p <= pos: a contiguous stretch of the list, at most w long;
 *   - within a row the values are ascending; a row with no record is in no run;
 *   - a covered row continues the run of the covered row before it only if the two rows are adjacent (i == prev + 1), both carry exactly one value, and it is
 *     the same value; otherwise it starts a run; a run's values are those of its first row.
 * The output is the argument set of rbg_set_markers: inclusive run_start[nruns], run_end[nruns], mk_off[nruns + 1], mk_vals[nvals].
 * Both calls take no handle and run on the current device.  d_sa: n entries of pos_bytes (rbg_suffix_array_dev's); d_pos, d_first, d_val: S u64 each (may be
 * NULL when S == 0); d_tmp: rbg_marker_runs_tmp_bytes(n, S, w, pos_bytes) bytes, 256-byte aligned -- 256 + n / 8 + n / 32 + 32 * min(n, S * w) bytes and
 * hipCUB's own, no array of n positions (0 = arguments no plan takes).  Nothing outside d_tmp and the outputs is written.
 * rbg_marker_runs_plan_dev: checks the rule about the records on the device, finds the covered rows and numbers the runs in d_tmp; *nruns, *nvals = the
 * sizes of the output.  It reads d_val, because whether two rows share a run depends on their values.  Waits for `stream`.
 * rbg_marker_runs_fill_dev, with the same arguments and d_tmp and the plan's counts: writes the four arrays.  It reads the plan's header back from d_tmp
 * (one wait for `stream`), then queues its kernel and returns.  d_sa, d_pos and d_first are checked but not read again.
 * RBG_EARG, nothing written to the outputs: n == 0, w outside 1..64, S > n, a NULL or misaligned pointer (d_tmp to 256, d_sa to pos_bytes, the rest to 8),
 * too little scratch, a pos_bytes that is not 4 or 8 or does not hold n, records that break the rule (plan), a d_tmp that does not hold the plan of these
 * n, S, w, pos_bytes, or counts that are not that plan's (fill).  S == 0 is RBG_OK with *nruns = *nvals = 0, and the fill then writes mk_off[0] = 0 only. */
size_t rbg_marker_runs_tmp_bytes(uint64_t n, uint64_t S, uint32_t w, uint32_t pos_bytes);
int rbg_marker_runs_plan_dev(const void *d_sa, uint64_t n, uint32_t pos_bytes, const uint64_t *d_pos, const uint64_t *d_first, const uint64_t *d_val, uint64_t S,
                             uint32_t w, void *d_tmp, size_t tmp_bytes, uint64_t *nruns, uint64_t *nvals, void *stream);
int rbg_marker_runs_fill_dev(const void *d_sa, uint64_t n, uint32_t pos_bytes, const uint64_t *d_pos, const uint64_t *d_first, const uint64_t *d_val, uint64_t S,
                             uint32_t w, const void *d_tmp, size_t tmp_bytes, uint64_t nruns, uint64_t nvals, uint64_t *d_run_start, uint64_t *d_run_end,
                             uint64_t *d_mk_off, uint64_t *d_mk_vals, void *stream);
/* rbg_build_from_text / rbg_convert_text with the marker pass run while the suffix array is still on the device: the records (host memory) are uploaded, the
 * two calls above run in the build's own scratch, and the arrays go on through rbg_set_markers / rbg_convert_runs_markers.  The scratch of the pass and 24
 * bytes per record are part of the bytes compared with hipMemGetInfo before anything is allocated; the marker arrays (16 bytes per run, 8 per value) are
 * checked once the plan has counted them.  RBG_EARG also for records that break the rule or w outside 1..64.  With S == 0 the calls are rbg_build_from_text
 * / rbg_convert_text exactly (pos, first, val and w are not looked at). */
int rbg_build_from_text_markers(const uint8_t *text, uint64_t n, const uint64_t *pos, const uint64_t *first, const uint64_t *val, uint64_t S, uint32_t w, int flags,
                                int device, rbg_index **out);
int rbg_convert_text_markers(const uint8_t *text, uint64_t n, const uint64_t *pos, const uint64_t *first, const uint64_t *val, uint64_t S, uint32_t w,
                             const char *docs_text /* nullable */, int flags, int device, const char *out_path);
/* ---- rb_markers' report (what the tool prints), made on the device --------------------------------------------------------------
 * Everything rb_markers does between get_markers_greedy_seeding / get_markers_lmems and its output (rb_markers.cpp:228-315, :365-382,
 * :396-413, :429-519), for a batch of RAW reads: both strands (sequence 2i = read i through seq_ntoa_table -- ACGT of either case, N/n -> 'A',
 * any other byte -> 'N' --, 2i + 1 = its reverse complement), the seeding, per callback record the min_range gate, the marker_cmp sort and
 * std::unique of its markers and (heuristic mode) clear_if_conflicting(read_len) and filter_identical_pos, then per read the records that
 * are printed, in print order: default mode forward then reverse; heuristic mode the strand first_fwd[i] names first (NULL: forward), the
 * other one only if the first did not set the stop rule, best-strand-only and min-seed-length as the reference applies them.  A record
 * with an empty range is never printed.  The coin (one std::mt19937 bit stream over the whole input) stays with the caller. */
#define RBG_REPORT_LMEM 1u               /* seed through get_markers_lmems (needs ftab_k > 0) instead of get_markers_greedy_seeding */
#define RBG_REPORT_HEURISTIC 2u          /* worker_heuristic (min_seed_len, the flags below) instead of worker */
#define RBG_REPORT_BEST_STRAND 4u
#define RBG_REPORT_CLEAR_CONFLICTING 8u
#define RBG_REPORT_CLEAR_IDENTICAL 16u
typedef struct rbg_report_params {
    uint64_t wsize, max_range, min_range, ftab_k, read_len, min_seed_len;
    uint32_t flags;   /* RBG_REPORT_LMEM | _HEURISTIC | _BEST_STRAND | _CLEAR_CONFLICTING | _CLEAR_IDENTICAL */
} rbg_report_params_t;
typedef struct rbg_report_seed { uint64_t range_size, query_start, query_len, mk_begin, mk_end; uint32_t strand /*0 +, 1 -*/, pad; } rbg_report_seed_t;
/* seed_off[N+1]: read i prints records [seed_off[i], seed_off[i+1]) of *seeds; a record's markers are (*mk)[mk_begin, mk_end), sorted and unique,
 * *mk dense in print order.  Both through rbg_free_buffer.  A line of rb_markers is
 *     <name> <range_size> <+|-> <query_start> <query_len> { " <seq>/<pos>/<allele>" per marker | " ." } "\n".
 * RBG_EARG: ftab_k - 1 > wsize (rowbowt.hpp:423-426), RBG_REPORT_LMEM with ftab_k == 0 (:346-349), unknown flags.  A read shorter than ftab_k in
 * greedy mode: its first lookup is a miss (see rbg_get_markers_greedy_seeding).  Works without a marker array (no record has markers).  A large
 * batch is walked in passes of bounded device memory (greedy: 64 MiB of reads, lmem: 4 Mi records; RBG_REPORT_CHUNK=<read bytes> overrides). */
int rbg_markers_report(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N, const uint8_t *first_fwd /* nullable */,
                       const rbg_report_params_t *params, uint64_t *seed_off, rbg_report_seed_t **seeds, uint64_t **mk);
/* The same as text, the lines written by kernels: names are N spans of name_base; *text is one of the handle's pinned text buffers, owned as
 * rbg_align_text's (rbg_wait_text before the first byte is read, rbg_release_text after, rbg_reserve_text to pin ahead of the clock).  An empty
 * report gives *text = NULL, *text_len = 0. */
int rbg_markers_report_text(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N, const uint8_t *first_fwd /* nullable */,
                            const rbg_report_params_t *params, const char *name_base, const uint64_t *name_begin, const uint32_t *name_len,
                            const char **text, uint64_t *text_len);
/* ---- the marker tally: per marker, how many of rb_markers' lines carried it ---------------------------------------------------------
 * For a caller who wants the genotyping evidence and not the lines.  Take the lines rbg_markers_report_text makes for a batch and an
 * rbg_report_params_t; for every line and every marker m on it: n_fwd[m] += 1 if the line's strand is '+', else n_rev[m] += 1, and
 * len_sum[m] += the line's query_len (wrapping).  A line with " ." adds nothing; a marker printed on two lines of one read counts twice (LINE
 * MODE, the default; PER-READ MODE below counts it once).  A marker is the full 64-bit value: every value is a legal key, 0 and 2^64 - 1 included.  The sums are of integers,
 * so the result does not depend on read order, on how the reads are split into calls and passes, or on the order in which the device's atomic
 * additions arrive: it is bit-reproducible.
 *
 * The table lives on the index's device (an open-addressing table of 32-byte slots, k_tally.hip) and is fed across passes, calls and batches;
 * nothing but the scalars a pass reads anyway comes back to the host until rbg_tally_export.  Its allocations are the index's: rbg_info().hbm_bytes
 * counts them.  FREE THE TALLY BEFORE ITS INDEX.  One tally may be fed by any number of calls one after another, NOT concurrently from two threads
 * (the host side keeps the reserve bookkeeping without a lock); separate tallies are independent.
 *
 * rbg_tally_create: capacity = max(64, the power of two >= 2 * distinct_hint) slots.  rbg_tally_reset: empty, the capacity kept.
 * rbg_tally_reserve: room for `extra` more elements at a load factor of at most 1/2; the host tracks an upper bound of the entries (every element
 * handed to a launch counts as a new one) and only when that bound says the room is missing does the call synchronise the device, read the
 * exact count and, if need be, grow (a larger table, every live slot re-inserted).
 * rbg_tally_add_dev: the records k_report_select left on the device (rbg_report_select_dev's d_out, R of them) and the marker array they point
 * into; M_upper >= the sum of their marker counts (mk_end - mk_begin) -- it sizes the launch and MUST NOT be less.  Asynchronous on `stream`
 * (the handle's element map grows, synchronising, when a call needs a larger one than any before); RBG_EARG, and nothing launched, when M_upper
 * exceeds the reserved room (capacity / 2 - the bound): reserve first.  d_tmp: rbg_tally_add_tmp_bytes(R), 8-byte aligned.
 * rbg_markers_tally: rbg_markers_report's arguments and checks; the lines' markers are added to the tally instead of being returned.
 * rbg_tally_add_entries: the export of another tally (another GPU's or rank's) added in: the merge.  Entries without counts add nothing.
 * rbg_tally_export: the entries with n_fwd + n_rev > 0, sorted by (sequence, position, allele); through rbg_free_buffer.
 * rbg_tally_info: {entries, capacity, grows since create / reset, records added, elements added, elements dropped}; dropped stays 0 -- a probe
 * sequence is bounded by the capacity and the reserve rule keeps the table half empty, the counter is the backstop's.
 * RBG_TALLY_COMBINE=0 (environment) turns off the combining of equal keys within a wave, for A/Bs: same result.
 *
 * PER-READ MODE (tally_flags = RBG_TALLY_PER_READ): the unit of evidence is the read.  Take one read and the lines printed for it, in print order.
 * For each DISTINCT marker m on them, the line carrying m with the greatest query_len -- the earliest such line on a tie -- adds: +1 to n_fwd[m] or
 * n_rev[m] by that line's strand, + its query_len to len_sum[m].  The read's other lines add nothing for m.
 * RBG_TALLY_DROP_SITE_CONFLICTS (only together with RBG_TALLY_PER_READ, RBG_EARG otherwise): a site is the marker without its allele -- bits 0-59,
 * sequence and position; the allele is bits 60-63.  A read whose lines carry two or more different alleles of one site, on one line or over several,
 * adds nothing for any marker of that site.  Every 64-bit value stays a legal marker: 2^64 - 1 is allele 15 of site (0xFFF, 2^48 - 1).
 * The additions are still sums of integers, so the export does not depend on read order, on the split into calls and passes (a pass holds whole
 * reads) or on the order of the atomics.  Line-mode and per-read adds may go into one tally; what such a mixture means is the caller's business.
 * rbg_markers_tally_reads: rbg_markers_tally with a flag word; 0 is rbg_markers_tally exactly, unknown bits give RBG_EARG.
 * rbg_tally_add_reads_dev: rbg_tally_add_dev plus the records' per-read offsets d_rep_off[N + 1] (rbg_report_select_dev's d_rep_off: read i printed
 * records [d_rep_off[i], d_rep_off[i + 1]), d_rep_off[N] = R), its checks and its reserve rule; R = 0 or N = 0 adds nothing.  tally_flags = 0 is
 * line mode.  d_tmp: rbg_tally_add_reads_tmp_bytes(N, R), 8-byte aligned.  PRECONDITION: every record's markers [mk_begin, mk_end) are ascending in
 * rotl64(marker, 4) and unique, as rbg_marker_seeds_canon_dev leaves them.  Markers that are not give an unspecified table, never an access outside
 * [mk_begin, mk_end).
 * rbg_tally_read_info: {reads seen by per-read adds, marker elements (of printed records) seen by them, elements that lost to another line of their
 * read, elements dropped by the site rule -- every copy counted}; seen = added + lost + dropped, where added is what these adds contribute to
 * rbg_tally_info's `elements` (which counts the elements actually added, in either mode; `records` the printed records handed in).  The counters'
 * device memory is allocated by the first per-read add (a tally that never sees one stays at its create-time allocations), counted in hbm_bytes,
 * zeroed by rbg_tally_reset and freed with the tally. */
#define RBG_TALLY_PER_READ 1u
#define RBG_TALLY_DROP_SITE_CONFLICTS 2u /* RBG_EARG without RBG_TALLY_PER_READ */
typedef struct rbg_tally rbg_tally;
typedef struct rbg_tally_entry { uint64_t marker, n_fwd, n_rev, len_sum; } rbg_tally_entry_t;
int rbg_tally_create(rbg_index *, uint64_t distinct_hint, rbg_tally **out);
void rbg_tally_free(rbg_tally *);
int rbg_tally_reset(rbg_tally *);
int rbg_tally_reserve(rbg_tally *, uint64_t extra);
size_t rbg_tally_add_tmp_bytes(uint64_t R);
int rbg_tally_add_dev(rbg_tally *, const rbg_report_seed_t *d_recs, uint64_t R, const uint64_t *d_mk, uint64_t M_upper, void *d_tmp, size_t tmp_bytes,
                      void *stream);
int rbg_markers_tally(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N, const uint8_t *first_fwd /* nullable */,
                      const rbg_report_params_t *params, rbg_tally *);
int rbg_tally_add_entries(rbg_tally *, const rbg_tally_entry_t *entries, uint64_t count);
int rbg_tally_export(rbg_tally *, uint64_t *count, rbg_tally_entry_t **entries);
int rbg_tally_info(rbg_tally *, uint64_t out[6]);
int rbg_markers_tally_reads(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N, const uint8_t *first_fwd /* nullable */,
                            const rbg_report_params_t *params, uint32_t tally_flags, rbg_tally *);
size_t rbg_tally_add_reads_tmp_bytes(uint64_t N, uint64_t R);
int rbg_tally_add_reads_dev(rbg_tally *, const rbg_report_seed_t *d_recs, uint64_t R, const uint64_t *d_rep_off /* [N+1] */, uint64_t N,
                            const uint64_t *d_mk, uint64_t M_upper, uint32_t tally_flags, void *d_tmp, size_t tmp_bytes, void *stream);
int rbg_tally_read_info(rbg_tally *, uint64_t out[4]);
/* ---- queries, device-resident buffers (HBM in, HBM out; asynchronous on `stream`) ---------- */
/* d_seqs: the reads back to back as in the host calls, in device memory, 16-BYTE ALIGNED (RBG_EARG otherwise), and the allocation must reach the next
 * multiple of 16 bytes at or past its last read's end: the kernels fetch reads as aligned 16-byte chunks (the bytes beyond a read's end are never used).
 * d_off[N + 1]: byte offsets.  Same answers as the host calls (find_range rowbowt.hpp:121-131, find_range_w_toehold :169-184); nothing is allocated, nothing
 * synchronised: graph-capturable.  A workspace, scratch or log area declared smaller than its size function reports (tmp_bytes, ws_bytes, log_bytes) is
 * answered with RBG_EARG before anything is enqueued: no output is touched. */

int rbg_find_range_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N,
                       uint64_t *d_lo, uint64_t *d_hi, void *stream);
int rbg_find_range_w_toehold_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N,
                                 uint64_t *d_lo, uint64_t *d_hi, uint64_t *d_ssamp, void *stream);
/* Packed reads: the same searches over a 2-bit form of the batch.  One lane per read fetching its
 * own bytes is 7 uncoalesced 16-byte requests per 100 bp; rbg_pack_reads_dev reads the bytes once,
 * coalesced, and writes every read as 2-bit codes in consumption order (64 symbols per 16 bytes)
 * into the caller's workspace; the *_packed_dev searches then take ceil(len/64) requests per read and
 * give the same results as rbg_find_range_dev / rbg_find_range_w_toehold_dev.  Reads with a symbol
 * outside the index's 4 most frequent symbols are searched from the bytes (pass the same d_seqs /
 * d_off).  total_bytes: any upper bound on d_off[N], the same in all three calls;
 * total_bytes/64 + N must stay below 2^32.  Measured on the bench batch (10 M x 100 bp): pack 0.8 ms,
 * searches 0.45-0.55 ms faster each -- worth it when a resident batch is searched more than once. */
size_t rbg_pack_ws_bytes(uint64_t N, uint64_t total_bytes);
int rbg_pack_reads_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t total_bytes,
                       void *d_ws, size_t ws_bytes, void *stream);
int rbg_find_range_packed_dev(rbg_index *, const void *d_ws, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N,
                              uint64_t total_bytes, uint64_t *d_lo, uint64_t *d_hi, void *stream);
int rbg_find_range_w_toehold_packed_dev(rbg_index *, const void *d_ws, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N,
                                        uint64_t total_bytes, uint64_t *d_lo, uint64_t *d_hi, uint64_t *d_ssamp, void *stream);
/* locate, two-phase because the output is ragged:
 *  1. rbg_locate_plan_dev writes d_loc_off[N+1]; d_tmp/tmp_bytes is scratch (query the size with
 *     rbg_locate_plan_tmp_bytes).  Read d_loc_off[N] to size d_locs.
 *  2. (optional) rbg_locate_order_dev; 3. rbg_locate_fill_dev walks the phi chains into d_locs. */
size_t rbg_locate_plan_tmp_bytes(uint64_t N);
int rbg_locate_plan_dev(rbg_index *, const uint64_t *d_lo, const uint64_t *d_hi, uint64_t N, uint64_t max_hits,
                        uint64_t *d_loc_off, void *d_tmp, size_t tmp_bytes, void *stream);
/* Optional, any time before fill: order the phi chains by toehold text position.  Chains of reads
 * from nearby loci visit the haplotypes in the same order, so neighbouring lanes then touch
 * neighbouring slots for the whole walk (k_locate_fill 9 -> 2.3 ms per 10M reads on the bench
 * index; the sort costs 0.36 ms).  Results are unchanged.  d_ws: 256-byte aligned, N < 2^32-1. */
size_t rbg_locate_order_ws_bytes(uint64_t N);
int rbg_locate_order_dev(rbg_index *, const uint64_t *d_k, uint64_t N, void *d_ws, size_t ws_bytes, void *stream);
/* d_order: the workspace prepared by rbg_locate_order_dev for the same d_k, or NULL (input order).
 * With d_order the walk takes each read's toehold from the workspace (it travelled with the sort) and
 * its count from d_loc_off (rbg_locate_plan_dev with the same max_hits): d_lo/d_hi are then not read.  d_k is: a toehold
 * that wrapped below zero has no place in the sorted keys and the walk reads d_k[i] for it (rbg_chain_walk.hpp chain_toehold), so
 * d_k must stay valid and UNCHANGED from rbg_locate_order_dev until the fill; and rbg_set_docs must not fall between the two
 * (the order's keys are made from the document table attached when it ran, and the fill decodes them with the current one).
 * d_locs needs 8-byte alignment only: the walk stores whole 64-byte windows of the array wherever it starts. */
int rbg_locate_fill_dev(rbg_index *, const uint64_t *d_lo, const uint64_t *d_hi, const uint64_t *d_k, uint64_t N,
                        uint64_t max_hits, const uint64_t *d_loc_off, uint64_t *d_locs, const void *d_order, void *stream);
/* locate_fill with a per-read value subtracted from every location (d_sub nullable): the
 * `locs[i] - best_range.qstart` of locate_from_longest_seed, rowbowt.hpp:681-683 */
/* The same walk storing each location as 32 bits (d_loc_off still counts locations): for device pipelines on an
 * index with 4-byte positions (rbg_info().pos_bytes == 4, i.e. n < 2^32 - 16; RBG_EARG otherwise) -- half the write
 * requests of the step that dominates count+locate.  The values are the low 32 bits of rbg_locate_fill_dev's, so a
 * toehold that wrapped below zero (a match at text position 0 of a range wider than one row) reads 0xFFFFFFFF.
 * The host API and the reference's signature (vector<uint64_t>, toehold_sa.hpp:37-49) keep 64 bits. */
int rbg_locate_fill_dev32(rbg_index *, const uint64_t *d_lo, const uint64_t *d_hi, const uint64_t *d_k, uint64_t N,
                          uint64_t max_hits, const uint64_t *d_loc_off, uint32_t *d_locs32, const void *d_order, void *stream);
int rbg_locate_fill_offset_dev(rbg_index *, const uint64_t *d_lo, const uint64_t *d_hi, const uint64_t *d_k, uint64_t N,
                               uint64_t max_hits, const uint64_t *d_loc_off, uint64_t *d_locs, const uint64_t *d_sub,
                               const void *d_order, void *stream);
int rbg_greedy_longest_seed_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t min_length,
                                uint64_t *d_lo, uint64_t *d_hi, uint64_t *d_qstart, uint64_t *d_qend, uint64_t *d_ssamp,
                                void *stream);
/* marker seeds, two-phase: plan writes the exclusive scans d_seed_off[N+1] (records per read) and
 * d_mk_off[N+1] (markers per read); the caller sizes d_seeds / d_mk from their last entries. */
int rbg_marker_seeds_plan_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t wsize,
                              uint64_t max_range, uint64_t ftab_k, uint64_t *d_seed_off, uint64_t *d_mk_off, void *d_tmp, size_t tmp_bytes,
                              void *stream);
int rbg_marker_seeds_fill_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t wsize,
                              uint64_t max_range, uint64_t ftab_k, const uint64_t *d_seed_off, const uint64_t *d_mk_off,
                              rbg_marker_seed_t *d_seeds, uint64_t *d_mk, void *stream);
/* The same two phases with a LOG between them, so that the reads are walked once: the plan also writes, per sequence, its
 * seed records and where its markers sit in the marker array into d_log (rbg_marker_seeds_log_bytes(ix, N, q) bytes for a
 * quota of q seeds per sequence, 0 = the default 12; 16-byte aligned; any larger area raises the quota), the fill copies
 * from there and walks only the sequences that exceeded their quota (listed at the log's end).  Same outputs as the pair
 * above; d_seeds 16-byte aligned; d_log must be left untouched between the two calls.  On the bench index the pair
 * takes 43 ms per 10 M reads (both strands) walking twice and about half with the log. */
size_t rbg_marker_seeds_log_bytes(const rbg_index *, uint64_t N, uint32_t seeds_per_read);
int rbg_marker_seeds_plan_log_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t wsize,
                                  uint64_t max_range, uint64_t ftab_k, uint64_t *d_seed_off, uint64_t *d_mk_off, void *d_tmp,
                                  size_t tmp_bytes, void *d_log, size_t log_bytes, void *stream);
int rbg_marker_seeds_fill_log_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t wsize,
                                  uint64_t max_range, uint64_t ftab_k, const uint64_t *d_seed_off, const uint64_t *d_mk_off,
                                  rbg_marker_seed_t *d_seeds, uint64_t *d_mk, void *d_log, size_t log_bytes, void *stream);
/* lmem marker seeds (rbg_get_markers_lmems), two-phase.  total: any upper bound on d_off[N] - d_off[0] (the number of records).
 * d_tmp: rbg_marker_lmems_tmp_bytes(N, total) bytes, 8-byte aligned: the plan leaves every record's marker offset there and the
 * fill reads it, so d_tmp must be left untouched between the two calls.  The plan writes d_mk_off[N+1], the exclusive scan of
 * the markers per sequence (d_mk_off[N] sizes d_mk); the fill writes record k of sequence i at d_seeds[d_off[i] - d_off[0] + k]
 * (caller provides (d_off[N] - d_off[0]) * 48 bytes) and the markers (caller provides d_mk_off[N] * 8 bytes; NULL when 0). */
size_t rbg_marker_lmems_tmp_bytes(uint64_t N, uint64_t total);
int rbg_marker_lmems_plan_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t total, uint64_t wsize,
                              uint64_t max_range, uint64_t ftab_k, uint64_t *d_mk_off, void *d_tmp, size_t tmp_bytes, void *stream);
int rbg_marker_lmems_fill_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t total, uint64_t wsize,
                              uint64_t max_range, uint64_t ftab_k, const void *d_tmp, rbg_marker_seed_t *d_seeds, uint64_t *d_mk, void *stream);
/* greedy seed lists (rbg_get_seeds_greedy), two-phase.  The plan walks the reads without any toehold state and writes
 * d_seed_off[N+1], the exclusive scan of the seeds per read (d_tmp: rbg_greedy_seeds_tmp_bytes(N) bytes); the fill walks them again
 * (same min_length and flags) and writes record r of read i at index d_seed_off[i] + r of five arrays of d_seed_off[N] entries
 * each; d_ssamp may be NULL without RBG_SEEDS_W_SAMPLE (else it is written 0).  The arrays go unchanged into rbg_locate_plan_dev
 * (d_lo, d_hi), rbg_locate_order_dev (d_ssamp) and rbg_locate_fill_offset_dev (d_sub = d_qstart): "locate every seed of every
 * read" is these two calls and those.  A zero-length seed (min_length == 0) has the full range: give it to K3 with care. */
size_t rbg_greedy_seeds_tmp_bytes(uint64_t N);
int rbg_greedy_seeds_plan_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t min_length, uint32_t flags,
                              uint64_t *d_seed_off, void *d_tmp, size_t tmp_bytes, void *stream);
int rbg_greedy_seeds_fill_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t min_length, uint32_t flags,
                              const uint64_t *d_seed_off, uint64_t *d_lo, uint64_t *d_hi, uint64_t *d_qstart, uint64_t *d_qend,
                              uint64_t *d_ssamp, void *stream);
/* toehold checkpoints (rbg_find_range_w_toehold_chkpnts) on the device.  The records a read can have are a function of its length
 * and wsize alone, so there is no count walk: rbg_toehold_chkpnts_slots_dev writes d_slot_off[N+1], the exclusive scan of those
 * fixed slots (from d_off alone; d_tmp: rbg_toehold_chkpnts_tmp_bytes(N) bytes), and the one walk writes record r of read i at index
 * d_slot_off[i] + r of five arrays of d_slot_off[N] entries each, and d_cnt[i] = 0 (the read does not occur: its slots hold nothing
 * of use) or d_slot_off[i+1] - d_slot_off[i].  The host call compacts; a device caller skips the slots of reads with d_cnt[i] == 0.
 * RBG_ENOTLOADED without a toehold SA (the host call answers empty lists there); wsize == 0: RBG_EARG. */
size_t rbg_toehold_chkpnts_tmp_bytes(uint64_t N);
int rbg_toehold_chkpnts_slots_dev(rbg_index *, const uint64_t *d_off, uint64_t N, uint64_t wsize, uint64_t *d_slot_off, void *d_tmp,
                                  size_t tmp_bytes, void *stream);
int rbg_find_range_w_toehold_chkpnts_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t wsize,
                                         const uint64_t *d_slot_off, uint64_t *d_cnt, uint64_t *d_lo, uint64_t *d_hi,
                                         uint64_t *d_qstart, uint64_t *d_qend, uint64_t *d_ssamp, void *stream);
/* The device steps of rbg_markers_report.  rbg_read_strands_dev: d_seqs / d_off[N+1] as in the searches above (16-byte aligned, the allocation reaching the
 * next multiple of 16; d_off[0] need not be 0) -> the 2N-sequence batch d_seqs2 (16-byte aligned, rbg_read_strands_bytes(total_bytes) bytes, total_bytes
 * any upper bound on d_off[N] - d_off[0]: the layout the *_dev searches require) and d_off2[2N+1] (d_off2[2i] = 2 (d_off[i] - d_off[0]),
 * d_off2[2i+1] = d_off2[2i] + length of read i). */
size_t rbg_read_strands_bytes(uint64_t total_bytes);
int rbg_read_strands_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t total_bytes, uint8_t *d_seqs2, uint64_t *d_off2,
                         void *stream);
/* In place over what rbg_marker_seeds_fill[_log]_dev / rbg_marker_lmems_fill_dev leave: for every record the survivors of {range_size >= min_range gate,
 * marker_cmp sort, unique, and by flags (RBG_REPORT_CLEAR_CONFLICTING, RBG_REPORT_CLEAR_IDENTICAL; others ignored) clear_if_conflicting(read_len) and
 * filter_identical_pos} end up at d_mk[mk_begin, mk_begin + c) and mk_end = mk_begin + c; what lies in the rest of the record's own stretch is
 * unspecified, no other byte of d_mk is written.  Segments may be of any length (S < 2^32).  d_tmp: rbg_marker_seeds_canon_tmp_bytes(S) bytes, 4-byte
 * aligned.  A group of 4, 16 or 64 lanes sorts a short segment (the width chosen on the device from the mean length, or forced by the environment
 * variable RBG_REPORT_GROUP for tests and A/Bs), longer segments get a workgroup each; the result does not depend on the path. */
size_t rbg_marker_seeds_canon_tmp_bytes(uint64_t S);
int rbg_marker_seeds_canon_dev(rbg_index *, rbg_marker_seed_t *d_seeds, uint64_t S, uint64_t *d_mk, uint64_t min_range, uint32_t flags, uint64_t read_len,
                               void *d_tmp, size_t tmp_bytes, void *stream);
/* Per read the printed records in print order: d_seed_off[2N+1] = the records of every sequence of the 2N batch (rbg_marker_seeds_plan*_dev's scan; d_off2
 * itself for lmem seeds), d_off2[2N+1] from rbg_read_strands_dev, d_first_fwd[N] the coins (nullable).  params is a HOST pointer (read_len, min_seed_len
 * and flags are used).  Writes d_rep_off[N+1] (exclusive scan of the records per read), the records at d_out[d_rep_off[i] ...] (room for as many as
 * there are input records) and, when d_out_read != NULL, each record's read.  d_tmp: rbg_report_select_tmp_bytes(N). */
size_t rbg_report_select_tmp_bytes(uint64_t N);
int rbg_report_select_dev(rbg_index *, const rbg_marker_seed_t *d_seeds, const uint64_t *d_seed_off, const uint64_t *d_off2, uint64_t N,
                          const uint8_t *d_first_fwd, const rbg_report_params_t *params, uint64_t *d_rep_off, rbg_report_seed_t *d_out,
                          uint32_t *d_out_read, void *d_tmp, size_t tmp_bytes, void *stream);
/* markers, same two-phase shape */
int rbg_markers_plan_dev(rbg_index *, const uint64_t *d_lo, const uint64_t *d_hi, uint64_t N,
                         uint64_t *d_mk_off, void *d_tmp, size_t tmp_bytes, void *stream);
int rbg_markers_fill_dev(rbg_index *, const uint64_t *d_lo, const uint64_t *d_hi, uint64_t N,
                         const uint64_t *d_mk_off, uint64_t *d_mk, void *stream);
/* markers at located text positions (rbg_markers_at_locs), two-phase, over what K3 leaves on the device: d_locs as rbg_locate_fill_dev /
 * rbg_locate_fill_offset_dev write them (64-bit: rbg_locate_fill_dev32's output cannot hold a location that wrapped below zero and is not
 * taken), d_loc_off[N+1], and the reads' d_off[N+1] (only the lengths are used).  The plan writes d_mk_off[N+1], per read (d_tmp:
 * rbg_loc_markers_tmp_bytes(N) bytes -- nothing is stored per location); the fill writes the values.  A group of 4, 16 or 64 lanes walks one
 * read's locations; the width is chosen on the device from d_loc_off[N] / N, or forced by the environment variable RBG_LOCMK_GROUP (tests, A/Bs). */
size_t rbg_loc_markers_tmp_bytes(uint64_t N);
int rbg_loc_markers_plan_dev(rbg_index *, const uint64_t *d_locs, const uint64_t *d_loc_off, const uint64_t *d_off, uint64_t N,
                             uint64_t *d_mk_off, void *d_tmp, size_t tmp_bytes, void *stream);
int rbg_loc_markers_fill_dev(rbg_index *, const uint64_t *d_locs, const uint64_t *d_loc_off, const uint64_t *d_off, uint64_t N,
                             const uint64_t *d_mk_off, uint64_t *d_mk, void *stream);

/* ---- document hits: which documents a read's locations fall in, answered where the locations are ------------------------------------
 * On an index with one document per haplotype (rbg_set_docs, doclist.hpp:57-73) the question a location list answers is "which haplotypes carry this
 * read, and how many reads does each haplotype carry".  These calls answer it from K3's output on the device: a set of 50 documents is 8 bytes per read
 * where the locations are 37 x 8 on the bench index.  The rule is rbg_resolve_offset's (DocList::doc_and_offset_at doclist.hpp:46-50 over doc_bounds_rank :77-79): for a
 * position l, q = min(l + 1, size) with l + 1 wrapping at 2^64 and size = the LAST start given + 1 (doclist.hpp:66); j = # sorted starts < q; j == 0: no
 * document, else document j - 1 -- entry j - 1 of rbg_doc_table -- at offset l - sorted_starts[j - 1].
 * The device table holds at most RBG_DOCS_MAX documents (rbg_docs_prepare: RBG_EARG beyond). */
#define RBG_DOCS_MAX 65536u
#define RBG_DOC_NONE 0xFFFFFFFFu
/* doclist.hpp:46-50, :77-79.  Uploads the sorted starts and their directory (rowbowt_amd/csrc/rbg_docdir.hpp) to the handle's device; idempotent.
 * RBG_ENOTLOADED without documents.  A later rbg_set_docs drops the copy (prepare again; the *_dev calls below answer RBG_ENOTLOADED until then, on the
 * primary and on every replica of it).  A replica prepares its own copy from its primary's table.  Must not overlap queries on the handle, like
 * rbg_set_docs. */
int rbg_docs_prepare(rbg_index *);
/* doclist.hpp:46-50, :77-79.  W = ceil(ndocs / 64): the u64 words of one read's document set (bit d % 64 of word d / 64 = document d); 0 without documents */
size_t rbg_doc_hits_words(const rbg_index *);
/* doclist.hpp:46-50, :77-79 for M locations on the device, one per lane: d_doc[j] = the document of d_locs[j] or RBG_DOC_NONE, d_offset[j] (nullable) = its
 * offset in that document, or the location itself when it has none.  _dev32: locations as rbg_locate_fill_dev32 writes them; 0xFFFFFFFF stands for the
 * toehold that wrapped below zero, 2^64 - 1 (no document; its offset reads 2^64 - 1).  Asynchronous on `stream`, nothing allocated or synchronised;
 * RBG_ENOTLOADED without a prior rbg_docs_prepare. */
int rbg_resolve_offsets_dev(rbg_index *, const uint64_t *d_locs, uint64_t M, uint32_t *d_doc, uint64_t *d_offset /* nullable */, void *stream);
int rbg_resolve_offsets_dev32(rbg_index *, const uint32_t *d_locs32, uint64_t M, uint32_t *d_doc, uint64_t *d_offset /* nullable */, void *stream);
/* doclist.hpp:46-50, :77-79 reduced per read: read i has the locations d_locs[d_loc_off[i], d_loc_off[i + 1]) (K3's output).  d_sets[i * W ...]: the SET of their
 * documents; d_ndocs[i]: the number of distinct documents; d_nodoc[i]: the number of its locations that have no document; d_doc_reads[d] += 1 for every
 * document d of the set -- reads per document, a read counting once per document; it ACCUMULATES over calls (zero it first).  Every output is nullable.
 * A group of 4, 16 or 64 lanes walks one read; the width is chosen on the device from d_loc_off[N] / N, or forced by the environment variable
 * RBG_DOCS_GROUP (tests, A/Bs): the outputs do not depend on it.  Asynchronous on `stream`, nothing allocated or synchronised; RBG_ENOTLOADED without a
 * prior rbg_docs_prepare. */
int rbg_doc_hits_dev(rbg_index *, const uint64_t *d_locs, const uint64_t *d_loc_off, uint64_t N, uint64_t *d_sets /* [N * W] nullable */,
                     uint32_t *d_ndocs /* [N] nullable */, uint32_t *d_nodoc /* [N] nullable */, uint64_t *d_doc_reads /* [ndocs] nullable, ACCUMULATES */,
                     void *stream);
/* doclist.hpp:46-50, :77-79 over the output of rbg_locate_fill_dev32; 0xFFFFFFFF = the wrapped toehold = no document (counted in d_nodoc) */
int rbg_doc_hits_dev32(rbg_index *, const uint32_t *d_locs32, const uint64_t *d_loc_off, uint64_t N, uint64_t *d_sets /* [N * W] nullable */,
                       uint32_t *d_ndocs /* [N] nullable */, uint32_t *d_nodoc /* [N] nullable */, uint64_t *d_doc_reads /* [ndocs] nullable, ACCUMULATES */,
                       void *stream);
/* doclist.hpp:46-50, :77-79 for a batch of reads in host memory: rbg_find_range_w_toehold (lo, hi as that call writes them), rbg_locs_at with max_hits, and
 * the reduction above over its locations, which never leave the device -- per read 16 + 8 W + 4 (+ 4) bytes come back instead of 8 per location.  The batch
 * is searched in chunks of reads and located in pieces of a bounded number of locations, so the scratch on the device stays bounded; rbg_counters sees every
 * read and every location once.  Prepares the table itself if needed.  doc_reads accumulates into the
 * caller's array.  RBG_ENOTLOADED without the toehold SA or documents. */
int rbg_doc_hits(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t max_hits, uint64_t *lo, uint64_t *hi, uint64_t *sets /* [N * W] */,
                 uint32_t *ndocs /* [N] */, uint32_t *nodoc /* [N] nullable */, uint64_t *doc_reads /* [ndocs] nullable, accumulates */);
/* toehold_sa.hpp:37-49 walked, doclist.hpp:46-50 / :77-79 applied to every position, nothing stored per location: the outputs of rbg_locate_plan_dev +
 * rbg_locate_fill_dev + rbg_doc_hits_dev for the same arguments, bit for bit, from ONE kernel that walks each read's phi chain (one lane per read, as the fill)
 * and keeps the chain's document set in LDS.  d_lo, d_hi, d_k: rbg_find_range_w_toehold_dev's outputs; read i has min(hi - lo + 1, max_hits) locations.
 * d_order (nullable): the workspace rbg_locate_order_dev filled for the same d_k and N.  d_k must stay valid and UNCHANGED between rbg_locate_order_dev and this
 * call, as for the fill (the ordered walk reads d_k[i] itself for a toehold that wrapped below zero), and rbg_set_docs must not fall between the two (the
 * order's keys are made from the table attached when it ran).  d_sets, d_ndocs, d_nodoc, d_doc_reads: as rbg_doc_hits_dev.  d_doc_locs[d] += the number of
 * walked positions whose document is d (ACCUMULATES): over one call the sum of its increments plus the sum of d_nodoc is what rbg_counters' fourth value grows
 * by, which is what the fill would have added.  Every output is nullable; with every output NULL the walk still runs (the counters see it).  Asynchronous on
 * `stream`, nothing allocated or synchronised.  RBG_ENOTLOADED without the toehold SA or without a current rbg_docs_prepare (as rbg_doc_hits_dev; replicas
 * included); RBG_EARG above RBG_LOCATE_DOCS_MAX documents (the table must fit LDS: use the three calls above) and on a null d_lo / d_hi / d_k with N > 0. */
#define RBG_LOCATE_DOCS_MAX 1024u
int rbg_locate_doc_hits_dev(rbg_index *, const uint64_t *d_lo, const uint64_t *d_hi, const uint64_t *d_k, uint64_t N, uint64_t max_hits,
                            const void *d_order /* nullable */, uint64_t *d_sets /* [N*W] nullable */, uint32_t *d_ndocs /* [N] nullable */,
                            uint32_t *d_nodoc /* [N] nullable */, uint64_t *d_doc_reads /* [ndocs] nullable, ACCUMULATES */,
                            uint64_t *d_doc_locs /* [ndocs] nullable, ACCUMULATES */, void *stream);
/* rbg_doc_hits with one more output: doc_locs[d] += the locations of this batch that fall in document d (nullable, accumulates).  Both calls take the
 * same path: with at most RBG_LOCATE_DOCS_MAX documents each chunk of reads is searched, ordered and walked by rbg_locate_doc_hits_dev's kernel -- no
 * locations stored, no plan, no pieces.  Larger tables, RBG_DOC_HITS_FUSED=0 (A/B) and any setting of RBG_DOC_HITS_CHUNK_LOCS (it bounds the location
 * scratch, which only that path has) take the two-step path described above; the outputs and rbg_counters are the same either way. */
int rbg_doc_hits_locs(rbg_index *, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t max_hits, uint64_t *lo, uint64_t *hi,
                      uint64_t *sets /* [N * W] */, uint32_t *ndocs /* [N] */, uint32_t *nodoc /* [N] nullable */,
                      uint64_t *doc_reads /* [ndocs] nullable, accumulates */, uint64_t *doc_locs /* [ndocs] nullable, accumulates */);

/* ---- global counters (the values the 8-GPU run reduces over RCCL) -------------------------- */
/* {reads processed, reads matched (non-empty range), sum of occ, sum of located positions}
 * accumulated on the device by every query since load / the last reset. */
int rbg_counters(rbg_index *, uint64_t out[4]);
int rbg_counters_reset(rbg_index *);
/* One-read calls (N = 1) of rbg_find_range / rbg_count / rbg_find_range_w_toehold / rbg_get_markers_greedy_seeding
 * made concurrently by several host threads are combined into one batched launch per round: what lets a caller
 * written against the reference's one-query-at-a-time methods from a thread pool (its only parallel dispatcher:
 * rb_markers.cpp:318-535) get batched launches unmodified.  out = {launches, requests served by them} since load;
 * requests / launches is the mean batch size.  (Environment RBG_HOST_COMBINE=0 switches the combining off.) */
int rbg_combine_stats(rbg_index *, uint64_t out[2]);

/* ---- several GPUs (index replicated, read stream sharded, no data-path collective; the reference is
 * single-device, its only parallel dispatcher is rb_markers' thread pool, rb_markers.cpp:318-535) --------------- */
/* A further replica of `primary`'s device index on `device`: built once, copied peer to peer (hipMemcpyPeer over
 * xGMI), its pointer-bearing records re-pointed.  The handle works with every query entry point above (host or
 * *_dev), shares the host-side index with the primary and must be freed before it; markers / docs are attached
 * to the primary BEFORE replicating. */
int rbg_replicate(rbg_index *primary, int device, rbg_index **replica_out);
/* G replicas at once: every target's peer copies are enqueued (one stream per target) before any is waited for, so the
 * transfers overlap -- each MI355X has its own xGMI link to the primary, the fan-out takes about one copy's time.
 * All or nothing: on failure no replica is left behind.  devices[] may repeat (tests put several on one device). */
int rbg_replicate_many(rbg_index *primary, const int *devices, int G, rbg_index **replicas_out /* [G] */);
/* What the fan-out cost one replica (measurement plumbing of the multi-GPU start, SURVEY 8e's "one-time distribution by parallel
 * peer copies"; the reference has no counterpart): out = {milliseconds its copies took on its own stream (HIP events), bytes
 * copied, peer access to the primary's device (1 = direct, 0 = staged through the host by the runtime, -1 = same device)}. */
int rbg_replicate_stats(const rbg_index *replica, double out[3]);
/* What the check of the re-pointed copy found when this replica was made (no device work; RBG_EARG on a primary): a source word that points into the
 * primary's i-th allocation must be the replica's i-th allocation plus the same offset on the replica, every other word of DevIndex and of the DevSym records
 * must be bit-identical.  out = {words of DevIndex recognised as such pointers, words of DevIndex that break the rule, the same two over every record of the
 * pointer tables}.  A violation also went to stderr with its byte offset and kind; queries answer correctly either way (from the primary's memory over the
 * peer link, or by the path that does without the array), which is why this is a call and not an error of rbg_replicate. */
int rbg_replica_pointer_check(const rbg_index *replica, uint64_t out[4]);
/* contiguous block [begin, end) of `rank` out of `world` (sizes differ by at most one; concatenating the ranks'
 * outputs restores the input order): read i of N goes to rank i * world / N */
int rbg_shard_bounds(uint64_t n_items, int rank, int world, uint64_t *begin, uint64_t *end);
/* find_range (ssamp == NULL) / find_range_w_toehold over G replicas: shard g of the batch runs on replicas[g],
 * the G shards concurrently; outputs in input order. */
int rbg_find_range_sharded(rbg_index *const *replicas, int G, const uint8_t *seqs, const uint64_t *off, uint64_t N,
                           uint64_t *lo, uint64_t *hi, uint64_t *ssamp /* nullable */);
/* The run's only collective: one RCCL all-reduce (sum) of the four counters of rbg_counters.  `nccl_comm` is the
 * caller's ncclComm_t for this replica's device (one rank per GPU), `stream` a HIP stream or NULL. */
int rbg_counters_allreduce(rbg_index *, void *nccl_comm, void *stream, uint64_t out[4]);
/* the same for G replicas on G distinct devices held by one process: one grouped all-reduce over a communicator
 * clique that is made on the first call for that set of devices (ncclCommInitAll) and kept for the later ones;
 * rbg_comm_cache_clear() destroys the kept cliques.  RCCL itself is opened on the first call that needs it
 * (dlopen): librbg.so does not link it, and RBG_ENODEV is the answer where it is absent. */
int rbg_counters_allreduce_local(rbg_index *const *replicas, int G, uint64_t out[4]);
int rbg_comm_cache_clear(void);

/* ---- measurement: what a launch touched (SURVEY 8d "report mean executed steps"; the reference's only
 * instrumentation is the stderr timer line rb_align.cpp:192) ------------------------------------------ */
/* The *_stats_dev calls run an INSTRUMENTED instantiation of the same kernel on the same arguments (same
 * outputs, same counters) and add what it touched to a device array of RBG_SEARCH_STATS / RBG_LOCATE_STATS
 * 64-bit sums, which the caller zeroes first.  bench.py derives the bytes of the algorithm as run from them;
 * the timed launches are the plain ones. */
/* On the run-indexed layout (RBG_LAYOUT_RUNS) the same sums count that layout's accesses: RBG_SS_SLOTS = directory
 * gathers (8 bytes each), RBG_SS_DENSE = run-list entries the probes needed (2 positions' width each; at most 16 per
 * probe), RBG_SS_SEARCH = narrowing rounds of crowded buckets (16 pivot keys each), RBG_SS_RESAMPLE = one sample gather
 * each; RBG_LS_PHI_STEPS = phi evaluations (one 8-byte directory gather + one probe each), RBG_LS_PHI_SEARCH = sampled
 * positions those probes and their narrowing rounds needed. */
enum { RBG_SS_STEPS = 0,      /* LF gathers issued (single-symbol or k-mer steps) */
       RBG_SS_SLOTS,          /* 16-byte rank slots loaded (1 per step, 2 when lo and hi+1 fall in different buckets) */
       RBG_SS_DENSE,          /* 2-byte loads from dense overflow tables */
       RBG_SS_SEARCH,         /* ranks answered by a run-list search (overflow bucket without a dense table) */
       RBG_SS_FTAB,           /* ftab entries fetched */
       RBG_SS_RESAMPLE,       /* toehold re-samples materialised (2 gathers each) */
       RBG_SS_CHUNKS,         /* aligned 16-byte chunks of read bytes fetched */
       RBG_SS_SYMBOLS,        /* read symbols consumed = reference LF iterations covered */
       RBG_SEARCH_STATS };
enum { RBG_LS_PHI_STEPS = 0,  /* phi evaluations (one phi slot each) */
       RBG_LS_PHI_SEARCH,     /* of them: answered by a run-list search */
       RBG_LS_CHAINS,         /* reads with at least one location */
       RBG_LS_LOCS,           /* locations stored */
       RBG_LOCATE_STATS };
/* The seeding kernels' instrumented instantiations (run-indexed layout only; RBG_EARG elsewhere): RBG_SEED_STATS sums -- the eight of
 * RBG_SEARCH_STATS with that layout's meanings, then the marker side.  rbg_marker_seeds_stats_dev = rbg_marker_seeds_plan_dev +
 * rbg_marker_seeds_fill_dev (the two-walk pair, no log, no --ftab) with both walks instrumented: same offsets, records and markers. */
enum { RBG_SD_MARKER_QUERIES = 8, /* window queries that went to the marker runs (rowbowt.hpp:437-441 with range <= max_range) */
       RBG_SD_MARKER_DIR,         /* bucket records read for them (32 bytes each: one per end of the range, one when both ends share a bucket; with RBG_MK_REC=0
                                     directory entries, 4 bytes each) */
       RBG_SD_MARKER_PROBES,      /* run starts / ends read from the arrays (8 bytes each): only behind an overflowing bucket's record */
       RBG_SD_MARKER_OFF,         /* value offsets read from the array (8 bytes each): likewise */
       RBG_SD_MARKER_VALS,        /* marker values copied (8 read + 8 written each) */
       RBG_SD_SEED_RECS,          /* seed records written (48 bytes each) */
       RBG_SD_SEQUENCES,          /* sequences walked */
       RBG_SEED_STATS };
int rbg_greedy_longest_seed_stats_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t min_length,
                                      uint64_t *d_lo, uint64_t *d_hi, uint64_t *d_qstart, uint64_t *d_qend, uint64_t *d_ssamp,
                                      uint64_t *d_stats /* RBG_SEED_STATS */, void *stream);
int rbg_marker_seeds_stats_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t wsize, uint64_t max_range,
                               uint64_t *d_seed_off, uint64_t *d_mk_off, void *d_tmp, size_t tmp_bytes, rbg_marker_seed_t *d_seeds,
                               uint64_t *d_mk, uint64_t *d_stats /* RBG_SEED_STATS */, void *stream);
int rbg_find_range_stats_dev(rbg_index *, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t *d_lo,
                             uint64_t *d_hi, uint64_t *d_ssamp /* NULL = count-only kernel */,
                             uint64_t *d_stats /* RBG_SEARCH_STATS */, void *stream);
int rbg_locate_fill_stats_dev(rbg_index *, const uint64_t *d_lo, const uint64_t *d_hi, const uint64_t *d_k, uint64_t N,
                              uint64_t max_hits, const uint64_t *d_loc_off, uint64_t *d_locs, const void *d_order,
                              uint64_t *d_stats /* RBG_LOCATE_STATS */, void *stream);

/* Synthetic reads generated on the device (measurement plumbing for BASELINE.json configs[3], "1B synthetic 150 bp
 * reads": the host cannot feed them, and the reference has no generator -- its reads come from a FASTQ,
 * rb_align.cpp:169-178).  Counter-based: read g = first_read + i is a pure function of (seed, g): a haplotype
 * g_h < H, an offset in [0, L - m] inside it (text position g_h * unit + offset of a text laid out as H units of
 * `unit` symbols whose first L are the haplotype), and with probability sub_ppm / 1e6 one substituted base.
 * Writes N reads of m bytes at stride m into d_seqs (16-byte aligned), d_off[N+1], and (optional) each read's
 * text position.  Needs no index. */
int rbg_sample_reads_dev(const uint8_t *d_text, uint64_t unit, uint64_t H, uint64_t L, uint64_t m, uint64_t seed,
                         uint64_t first_read, uint64_t N, uint32_t sub_ppm, uint8_t *d_seqs, uint64_t *d_off,
                         uint64_t *d_start /* nullable */, void *stream);
/* The same reads (byte for byte, for the same seed) from the STRUCTURE of such a text instead of the text: a pangenome of
 * n = 3e11 symbols does not fit the HBM it would be sampled from.  Symbol (h, p) is d_base[p] (L bytes), or d_alt[j] when p
 * is variant site j (d_sites: S ascending offsets) and haplotype h carries the alternative allele (d_G[j * H + h] != 0).
 * d_site_dir (nullable): d_site_dir[b] = # sites below b << site_dir_shift, (L >> site_dir_shift) + 2 entries (S < 2^32): the first
 * site of a read is then found in its bucket instead of by a search over all sites. */
int rbg_sample_reads_pangenome_dev(const uint8_t *d_base, const uint64_t *d_sites, const uint8_t *d_alt, const uint8_t *d_G, uint64_t S,
                                   const uint32_t *d_site_dir, uint32_t site_dir_shift, uint64_t unit, uint64_t H, uint64_t L, uint64_t m,
                                   uint64_t seed, uint64_t first_read, uint64_t N, uint32_t sub_ppm, uint8_t *d_seqs, uint64_t *d_off,
                                   uint64_t *d_start /* nullable */, void *stream);

/* ---- tuning (never changes results) -------------------------------------------------------- */
/* Process-wide defaults read when an index is built/loaded: BLOCK_THREADS (64, 128, 192 or 256; the search
 * kernels use 1024-thread workgroups instead while the 5-mer level is resident),
 * RANK/PHI_BUCKET_SHIFT (-1 = automatic, else 0..8; RANK also 9..12 = wide buckets), DEEP_BUCKET_SHIFT (-1 = like
 * RANK, else the bucket shift of the 4-mer and deeper tables only, whose runs are sparse), POS_BYTES (0 = automatic, 4 or 8 to force a width),
 * KMER_STEPS (1..8, default 8: symbols the backward search consumes per step; the slot layout takes at most 5 of them per gather; 2.. build the k-mer
 * tables of DESIGN.md 2b -- each level is four times the tables of the one before, 218 GB in all for a
 * 2-Gbase index; 1 keeps the reference's one-symbol steps only; the deepest levels are dropped
 * automatically when the replica would not fit), HBM_BUDGET_MB (0 = A QUARTER of the free HBM -- three quarters until round 3; a drop-in library leaves the device to its caller unless told otherwise:
 * upper bound for the replica, deciding how many k-mer levels are kept.  ONE EXCEPTION, reported by rbg_layout_info().budget_raised and on stderr: under
 * RBG_LAYOUT_AUTO with no budget given, an index of so many runs that the quarter would leave it fewer than four symbols per step (r about 1e9) takes up
 * to three quarters -- and only on a device the load has to itself (at least nine tenths of it free: with the caller's own buffers, another replica or
 * another process already there the quarter stays); any explicit HBM_BUDGET_MB switches the exception off), FTAB_K (-1 = automatic (the longest word of at most 12 symbols with 4^k <= n/16),
 * 0 = no ftab, else the word length of the ftab built on the GPU at load time: the state after the
 * last FTAB_K symbols of a read is one gather; result-neutral like the reference's ftab,
 * rowbowt.hpp:124-125,726-758).
 * DENSE_OVERFLOW (1 = default): buckets with more run starts than a slot holds get a two-bytes-per-row table
 * (512 bytes per such bucket, about 1.2 % on top of the replica) so that their rank is one more load
 * instead of a search of the run list; 0 = search the run list.
 * PACKED_READS applies to the host-pointer search calls, at call time: how the reads cross PCIe -- 0 = as bytes,
 * 1 (default) = as 2-bit codes packed by CPU threads for batches of >= 4096 reads (a quarter of the bytes; reads
 * holding symbols outside the index's four k-mer symbols are searched from their bytes afterwards), 2 = always
 * as 2-bit codes.  (Packing a batch that is already in HBM is rbg_pack_reads_dev.)
 * RANK_LAYOUT: RBG_LAYOUT_AUTO (default): slot tables while those of every requested symbol per step (KMER_STEPS), at their
 * narrow buckets, fit the HBM budget; otherwise the run-indexed layout rather than slot tables with wider buckets or fewer
 * symbols per step (on the bench index at the default budget 1.35-1.47e9 count+locate reads/s from 12 GB at eight symbols per step,
 * against 1.26e9 from the 221 GB of five symbols per gather and 1.18e9 from the 59 GB of four: profiles/r05_bench.json) -- unless that does
 * not fit either (about 110 bytes per run).  RBG_LAYOUT_PREFER_SLOTS: slot tables with as many symbols per step as fit, the
 * run-indexed layout only when not even the single-symbol level does (the rule of rounds 2-3; the seeding kernels are a quarter faster
 * on slot tables).  rbg_info::rank_layout reports the outcome.
 * RBG_LAYOUT_SLOTS, RBG_LAYOUT_RUNS = the run-indexed layout: the run lists of the k-mer depths RUN_DEPTHS names (by default the
 * deepest KMER_STEPS asks for and the budget holds, half of it, a quarter of it ... and 1) with a directory or bucket records per
 * table, space proportional to r and nothing proportional to n; rank and phi are predecessor searches over the few entries of
 * one bucket by the lane that owns the query (rle_string::rank rle_string.hpp:131-161 / ToeholdSA::phi toehold_sa.hpp:56-72 keep
 * their O(r) shape). */
/* Environment switches (read at load or per call; none of them changes an answer -- they exist for A/B measurements
 * and for the tests that pin both sides):  RBG_PHI_PACKED=0 keeps 32-byte phi slots at 8-byte positions;
 * RBG_RANK_DIR_RUNS=<x> sets the runs per rank-directory bucket of the run-indexed layout (default 4), RBG_RUN_REC_PER=<x> the entries
 * per bucket record (default 2.5), RBG_PHI_DIR_PER=<x> the sampled positions per phi-directory bucket (default 1..2);
 * RBG_RUN_FILL_SHIFT / RBG_PHI_SUPER_SHIFT lower the filler distance / super-count spacing of 8-byte positions so that tests
 * meet both on small indexes;  RBG_HOST_THREADS, RBG_HOST_CHUNK_READS, RBG_HOST_DIRECT_OUT=0, RBG_HOST_COMBINE=0,
 * RBG_HOST_TRACE=1|2 tune / trace the host-pointer pipeline;  RBG_LAYOUT=auto|slots|runs|prefer-slots, RBG_RUN_DEPTHS,
 * RBG_KMER_STEPS, RBG_HBM_BUDGET_MB, RBG_FTAB_K, RBG_JUMP_K, RBG_JUMP2_K, RBG_RUN_PHI, RBG_RUN_REC give the options of the same names their initial values (for
 * the command-line tools, which keep the reference's flags; rbg_set_default_option overrides them);  RBG_JUMP_ABSENT_ENDS=0 lets no level of the jump table
 * count as complete (rbg_jump_info_t::complete; read at every load);  RBG_H2D_STAGED=0 uploads the big
 * arrays of a load by plain hipMemcpy;  RBG_VERBOSE=1 prints what the budget rule did and the seconds of every stage of a load. */
enum { RBG_OPT_BLOCK_THREADS = 1, RBG_OPT_RANK_BUCKET_SHIFT = 2, RBG_OPT_PHI_BUCKET_SHIFT = 3, RBG_OPT_POS_BYTES = 4,
       RBG_OPT_KMER_STEPS = 5, RBG_OPT_HBM_BUDGET_MB = 6, RBG_OPT_FTAB_K = 7, RBG_OPT_PACKED_READS = 8,
       RBG_OPT_DEEP_BUCKET_SHIFT = 9, RBG_OPT_DENSE_OVERFLOW = 10, RBG_OPT_RANK_LAYOUT = 11,
       /* 12, 13 and 15 were RBG_OPT_TREE_TOP_KB, RBG_OPT_SLOT_BYTES and RBG_OPT_RUN_FMT (retired with ABI 3: RBG_EARG) */
       RBG_OPT_RUN_DEPTHS = 14 /* run-indexed layout: bit d - 1 set = keep run lists for the k-mer depth d (bit 0 is implied; depths
                                  above the highest bit are not built).  A search step consumes the longest stretch a kept
                                  depth covers, so any set gives the same answers; the lists grow with the depth (DESIGN.md
                                  2c).  0 = default: the deepest depth RBG_OPT_KMER_STEPS asks for, half of it, a quarter of
                                  it ... and 1 (1, 2, 4, 8 of eight: whole reads go by eight symbols a step, a remainder takes
                                  one step per set bit); 0xFF keeps all eight; over budget the depths between the first and
                                  the deepest go before the deepest does.  rbg_info(): kmer_steps is the deepest depth kept,
                                  depth_runs[d - 1] is 0 for the depths left out */,
       RBG_OPT_RUN_PHI = 16 /* run-indexed layout -- how phi (toehold_sa.hpp:56-72) is answered: 1 = from the list of sampled positions
                                  through its directory (12-16 bytes per run: two dependent sectors per step); 2 = from direct-addressed phi SLOTS
                                  (the slot layout's PhiSlot records) whose buckets are about n / r rows wide, so that their number is proportional
                                  to r (about 54 bytes per run at 8-byte positions: one sector per step -- at pangenome scale K3 is bound by that
                                  count); 0 (default) = slots when the whole replica then stays within the HBM budget.  RBG_RUN_PHI gives the
                                  initial value; rbg_layout_info().phi_slots says what was built. */,
       RBG_OPT_RUN_REC = 17 /* run-indexed layout -- BUCKET RECORDS: 2 = every bucket of a table (about three entries wide) gets one aligned
                                  64-byte record holding its entries and the one before them (up to eleven in the compact form, six otherwise; a bucket with
                                  more holds twelve pivots into the run list instead: rbg_dev.h RunRec2), direct-addressed: a rank is ONE sector instead of a
                                  directory sector plus an unaligned stretch of the run list (K1/K2 on this layout are bound by that count); about
                                  21-26 bytes per entry on top of the run lists, which stay for crowded buckets and the samples; 1 = directories only;
                                  0 (default) = decided PER DEPTH, deepest first (where a search spends its steps): a depth gets records -- at 2.5, else 4,
                                  else 6 entries per bucket -- while the replica with them (and with the phi slots, which come first) stays within the HBM budget.  RBG_RUN_REC gives the initial
                                  value, RBG_RUN_REC_PER the entries per bucket; rbg_layout_info().rec_bytes says what was built, per depth. */,
       RBG_OPT_RUN_REC_DEPTHS = 18 /* with RBG_OPT_RUN_REC = 2: bit d - 1 = the k-mer depth d gets bucket records, the other kept depths keep their
                                  directories (0, the default: every kept depth).  An index of r = 1e9 runs has room for the records of its deepest depth
                                  but not of all (profiles/r05_pangenome_stream_r1e9.json).  RBG_RUN_REC_DEPTHS gives the initial value. */,
       RBG_OPT_EXTRACT_CHUNK = 20 /* rbg_extract: the bases per piece an interval is cut into before the upload (1 .. 2^30; default 128, the fastest of 64 .. 4096 in profiles/extract_rate.txt).  The result
                                  does not depend on it */,
       RBG_OPT_JUMP_K = 19 /* the jump table (rbg_jump_info): 0 = none, 16..64 = a table of that many symbols per key, -1 (default) = 60 symbols
                                  when the replica is larger than the device's 256 MB last-level cache and the table adds at most half of it, none otherwise.  RBG_JUMP_K gives the initial value. */,
       RBG_OPT_JUMP2_K = 21 /* level 2 of the jump table (rbg_jump_info_sized), built only where the first table is: 0 = none, 16..48 = that many more symbols, -1 (default) = 40
                                  where the first table is the automatic one of 60 symbols and both tables together add at most the replica, none otherwise.  RBG_JUMP2_K gives
                                  the initial value. */ };
int rbg_set_default_option(int opt, int64_t value);
/* the value a later load would use (so that a caller can change a knob for one load and put it back) */
int rbg_get_default_option(int opt, int64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* RBG_H */
