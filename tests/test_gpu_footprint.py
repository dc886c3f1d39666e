"""The FOOTPRINT of the device API (include/rbg.h, the *_dev entry points): every call gets its inputs, outputs and workspaces out of one guarded arena
(tests/arena.py) -- each output of exactly the size the header says the caller provides, each workspace of exactly what its size function returns, all at
the MINIMUM alignment the header allows and off every 64-byte line -- and afterwards no guard byte has changed, no input has changed, and the values are
the reference's, exactly: the oracle for search, locate and markers, tests/seeds_model.py and tests/lmem_model.py for the seed lists, tests/doc_hits_model.py
for the document calls, tests/rb_locs_model.py for the markers at located positions, tests/rb_markers_model.py's tables for the strands.  An overrun lands in
guard bytes of the same allocation, never in unmapped memory.  Undersized DECLARATIONS (the memory behind the pointer is always of full size) are refused
with RBG_EARG and leave outputs and guards alone.

The batch: 600 ragged reads of the synth index with substitutions plus the quirk reads of the family tests; every case runs on all of it and on its first
1, 63, 64, 65 and 257 reads; on the slot layout and the run-indexed one at 4- and 8-byte positions.  The references are computed once per module
(about 2 s); with 600 reads the slowest case takes 0.6 s on an MI355X, the whole file 15 s.
The report's canon and select, the tally adds and the three walks (56-byte records at 4-byte alignment) have their own batches, described at their tests.
Alignment / skew of the outputs: u64 arrays 8 / 8 (d_locs also 8 / 56), u32 arrays and 32-bit locations 4 / 4, rbg_marker_seed_t records 8 / 8 (16 / 16
for the logged fill), d_seqs, d_seqs2, the pack workspace and the seed log 16 / 16, the order workspace 256 / 0, scratch areas 8 / 8."""
import os

import numpy as np
import pytest

import doc_hits_model as DM
import orc
import rb_markers_model as RM
import rowbowt_amd as ra
from arena import Arena
from lmem_model import lmem_records
from rb_locs_model import markers_at_loc
from rowbowt_amd import capi
from seeds_model import chkpnt_count, longest_seed, seeds_greedy, toehold_chkpnts
from test_gpu_loc_markers import _arrays, _grid_runs
from test_rb_locs_model import text_oracle

pytestmark = pytest.mark.gpu

MAXU = 2**64 - 1
EARG = -4
FORMS = [(capi.LAYOUT_SLOTS, 4), (capi.LAYOUT_SLOTS, 8), (capi.LAYOUT_RUNS, 4), (capi.LAYOUT_RUNS, 8)]
FORM_IDS = ["slots-4", "slots-8", "runs-4", "runs-8"]
COUNTS = [600, 1, 63, 64, 65, 257]
MAX_HITS = (1, 7, 8, 9, 16, 17, MAXU)
MIN_LENGTH, WSIZE, MAX_RANGE, CHK_WSIZE, LOCMK_HITS = 5, 10, 1000, 10, 17
NDOCS = 70                         # no multiple of 64: a row of d_sets ends inside its second word
ARENA_BYTES = 12 << 20


def up16(x):
    return (x + 15) & ~15


class env:
    """an environment variable for the calls inside (the group widths are read at every launch)"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.prev = os.environ.pop(self.name, None)
        if self.value is not None:
            os.environ[self.name] = str(self.value)

    def __exit__(self, *exc):
        os.environ.pop(self.name, None)
        if self.prev is not None:
            os.environ[self.name] = self.prev
        return False


# ---- the batch and its references, once per module ----------------------------------------------------------------------------------------------------
class Ref:
    pass


@pytest.fixture(scope="module")
def ref(synth):
    S = synth
    R = Ref()
    R.S = S
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    ms, me, mo, mv = S.markers(wsize=10)
    o.set_markers(ms, me, mo, mv)
    R.markers = (ms, me, mo, mv)
    reads = S.sample_reads(594, 120, seed=20261, sub_rate=0.1, ragged=True)
    quirks = [b"", b"A", b"N", b"ACGTN", S.text[:40].tobytes().lower(), S.text[500:800].tobytes()]
    reads = reads[:3] + quirks + reads[3:]          # (the quirk reads inside every prefix but the first)
    assert len(reads) == COUNTS[0]
    R.reads = reads
    R.seqs, R.off = ra.pack_reads(reads)
    R.lo, R.hi, k = o.find_range_w_toehold_batch(R.seqs, R.off, nthreads=4)
    occ = np.where(R.hi >= R.lo, R.hi - R.lo + np.uint64(1), np.uint64(0)).astype(np.int64)
    # toeholds that wrapped below zero by one and by two, on chains of several locations (their first location is stored by its owner lane)
    multi = np.flatnonzero(occ >= 3)
    assert len(multi) >= 2 and multi[1] < 63 and occ.max() > 17
    R.k = k.copy()
    R.k_true = k
    R.k[multi[0]] = np.uint64(MAXU)
    R.k[multi[1]] = np.uint64(MAXU - 1)
    R.locs = {mh: o.locs_at_batch(R.lo, R.hi, R.k, mh, nthreads=4) for mh in MAX_HITS + (LOCMK_HITS,)}
    R.longest = [longest_seed(seeds_greedy(o, q, 10)) or (1, 0, 0, 0, 0) for q in reads]
    R.markers_at = [o.markers_at(int(l), int(h)) if h >= l else [] for l, h in zip(R.lo, R.hi)]
    R.marker_seeds = [o.markers_greedy_seeding(q, WSIZE, MAX_RANGE, 0) for q in reads]
    R.lmems = [lmem_records(o, q, WSIZE, MAX_RANGE, 0) for q in reads]
    R.seed_lists = {w: [seeds_greedy(o, q, MIN_LENGTH, w) for q in reads] for w in (True, False)}
    R.chkpnts = [toehold_chkpnts(o, q, CHK_WSIZE) for q in reads]
    R.o = o
    # the text-position marker table and its oracle
    R.text_runs = _grid_runs(S.n)
    ot = text_oracle(R.text_runs)
    woff, wlocs = R.locs[LOCMK_HITS]
    R.loc_markers = []
    for i, q in enumerate(reads):
        got = []
        for l in wlocs[int(woff[i]):int(woff[i + 1])]:
            got += markers_at_loc(ot, int(l), len(q))
        R.loc_markers.append(got)
    ot.close()
    assert sum(1 for w in R.loc_markers if w) > 100 and sum(len(w) for w in R.markers_at) > 100
    rng = np.random.default_rng(17)
    R.doc_starts = [0] + np.sort(rng.choice(np.arange(1, S.n - 1), size=NDOCS - 1, replace=False)).tolist()
    yield R
    o.close()


@pytest.fixture(scope="module")
def handles(ref):
    """one prepared handle per form, made when first asked for"""
    made = {}

    def get(form):
        if form not in made:
            S = ref.S
            layout, pos_bytes = form
            with capi.default_option(capi.OPT_RANK_LAYOUT, layout), capi.default_option(capi.OPT_POS_BYTES, pos_bytes):
                rb = ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0)
            assert rb.info().rank_layout == layout and rb.info().pos_bytes == pos_bytes
            rb.set_markers(*ref.markers)
            rb.set_text_markers(*_arrays(ref.text_runs))
            rb.set_docs([f"d{j}" for j in range(NDOCS)], ref.doc_starts)
            rb.docs_prepare()
            rb.fl_prepare()
            made[form] = rb
        return made[form]

    yield get
    for rb in made.values():
        rb.close()


# ---- one case: an arena with the first n reads in it -----------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, ref, n, pad_byte=0x00, pattern=0xA5, lead=0, arena_bytes=ARENA_BYTES):
        import torch
        self.torch = torch
        self.R, self.N = ref, n
        self.A = Arena(arena_bytes, device="cuda:0", pattern=pattern)
        self.L = ra.lib()
        self.st = torch.cuda.current_stream().cuda_stream
        self.inputs = []
        off = ref.off[:n + 1]
        self.total = int(off[n])
        # d_seqs reaches only to the next multiple of 16 past the last read; `lead` garbage bytes (a multiple of 16) before the first read make d_off[0] != 0
        body = np.full(up16(lead + self.total), pad_byte, np.uint8)
        body[lead:lead + self.total] = ref.seqs[:self.total]
        self.seqs = self.inp("d_seqs", body, 16)
        self.off = self.inp("d_off", off + np.uint64(lead))

    def inp(self, name, array, align=8, skew=None):
        r = self.A.carve_from(name, array, align, skew)
        self.inputs.append(name)
        return r

    def out(self, name, nbytes, align=8, skew=None):
        return self.A.carve(name, nbytes, align, skew)

    def u64(self, name, count, skew=None):
        return self.out(name, 8 * count, 8, skew)

    def sync_and_check(self):
        """after the calls: the guards are clean and every input is what it was"""
        self.torch.cuda.synchronize()
        self.A.check()
        for name in self.inputs:
            if self.A[name].saved is None:
                raise AssertionError(f"{name}: an input without a snapshot")
        self.A.assert_all_unchanged()

    def freeze(self, *more):
        """snapshot the inputs (and outputs of earlier calls that later calls only read)"""
        for name in self.inputs + list(more):
            self.A.snapshot(name)
        self.inputs += [m for m in more if m not in self.inputs]


def same(region, want, dtype=np.uint64):
    got = region.numpy(dtype)
    want = np.asarray(want, dtype=dtype)
    assert got.shape == want.shape, (region.name, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (region.name, "first difference at element", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]), bad.size)


def refused(c, *calls):
    """every call (function, arguments ...) answers RBG_EARG, and after a synchronize not a byte of the arena has changed"""
    before = c.A.buf.clone()
    for fn, *args in calls:
        assert fn(*args) == EARG, fn
    c.torch.cuda.synchronize()
    assert bool((c.A.buf == before).all().item())


def scan(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.uint64))]).astype(np.uint64)


cases = pytest.mark.parametrize("n", COUNTS)
forms = pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)


# ---- search ---------------------------------------------------------------------------------------------------------------------------------------------
@forms
@cases
@pytest.mark.parametrize("garbage", [0x00, 0xFF])
def test_search(ref, handles, form, n, garbage):
    """rbg_find_range_dev, rbg_find_range_w_toehold_dev, rbg_greedy_longest_seed_dev, rbg_pack_reads_dev + the two packed searches (total_bytes exact and
    a loose upper bound).  The padding behind the last read and -- garbage 0xFF -- every guard byte of the arena hold another byte: the answers are the
    oracle's either way (the bytes beyond a read's end are never used)."""
    rb, R = handles(form), ref
    c = Case(R, n, pad_byte=garbage, pattern=0xA5 if garbage == 0 else 0xFF)
    L, st, N = c.L, c.st, n
    seqs, off = c.seqs.ptr, c.off.ptr
    lo, hi = c.u64("d_lo", N), c.u64("d_hi", N)
    lo2, hi2, k2 = c.u64("d_lo_t", N), c.u64("d_hi_t", N), c.u64("d_ssamp_t", N)
    g = [c.u64("d_g_" + f, N) for f in ("lo", "hi", "qstart", "qend", "ssamp")]
    c.freeze()
    assert L.rbg_find_range_dev(rb.h, seqs, off, N, lo.ptr, hi.ptr, st) == 0
    assert L.rbg_find_range_w_toehold_dev(rb.h, seqs, off, N, lo2.ptr, hi2.ptr, k2.ptr, st) == 0
    assert L.rbg_greedy_longest_seed_dev(rb.h, seqs, off, N, 10, *(t.ptr for t in g), st) == 0
    packed = []
    for tag, bound in (("exact", c.total), ("loose", c.total + 1000)):
        wsb = int(L.rbg_pack_ws_bytes(N, bound))
        ws = c.out("d_pack_ws_" + tag, wsb, 16)
        o4 = [c.u64(f"d_p{tag}_{f}", N) for f in ("lo", "hi", "lo_t", "hi_t", "ssamp_t")]
        assert L.rbg_pack_reads_dev(rb.h, seqs, off, N, bound, ws.ptr, wsb, st) == 0
        assert L.rbg_find_range_packed_dev(rb.h, ws.ptr, seqs, off, N, bound, o4[0].ptr, o4[1].ptr, st) == 0
        assert L.rbg_find_range_w_toehold_packed_dev(rb.h, ws.ptr, seqs, off, N, bound, o4[2].ptr, o4[3].ptr, o4[4].ptr, st) == 0
        packed.append(o4)
    c.sync_and_check()
    wlo, whi, wk = R.lo[:N], R.hi[:N], R.k_true[:N]
    same(lo, wlo); same(hi, whi)
    same(lo2, wlo); same(hi2, whi); same(k2, wk)
    for j, t in enumerate(g):
        same(t, [w[j] for w in R.longest[:N]])
    for o4 in packed:     # (the byte search's oracle answers)
        same(o4[0], wlo); same(o4[1], whi); same(o4[2], wlo); same(o4[3], whi); same(o4[4], wk)
    # refusals: d_seqs at 8-byte alignment, the pack workspace declared one byte short and empty
    wsb = int(L.rbg_pack_ws_bytes(N, c.total))
    before = c.A.buf.clone()
    assert L.rbg_find_range_dev(rb.h, seqs + 8, off, N, lo.ptr, hi.ptr, st) == EARG
    assert L.rbg_find_range_w_toehold_dev(rb.h, seqs + 8, off, N, lo2.ptr, hi2.ptr, k2.ptr, st) == EARG
    assert L.rbg_greedy_longest_seed_dev(rb.h, seqs + 8, off, N, 10, *(t.ptr for t in g), st) == EARG
    pws, o4 = c.A["d_pack_ws_exact"].ptr, packed[0]
    assert L.rbg_pack_reads_dev(rb.h, seqs + 8, off, N, c.total, pws, wsb, st) == EARG
    assert L.rbg_find_range_packed_dev(rb.h, pws, seqs + 8, off, N, c.total, o4[0].ptr, o4[1].ptr, st) == EARG
    assert L.rbg_find_range_w_toehold_packed_dev(rb.h, pws, seqs + 8, off, N, c.total, o4[2].ptr, o4[3].ptr, o4[4].ptr, st) == EARG
    for declared in (wsb - 1, 0):
        assert L.rbg_pack_reads_dev(rb.h, seqs, off, N, c.total, c.A["d_pack_ws_exact"].ptr, declared, st) == EARG
    c.torch.cuda.synchronize()
    assert bool((c.A.buf == before).all().item())


# ---- locate ---------------------------------------------------------------------------------------------------------------------------------------------
@forms
@cases
def test_locate(ref, handles, form, n):
    """rbg_locate_plan_dev, rbg_locate_order_dev (workspace 256-aligned, of exact size), rbg_locate_fill_dev unordered and ordered with d_locs skewed by 8
    and by 56 (a window's head and tail both straddle lines), rbg_locate_fill_dev32 at 4-byte positions and its refusal at 8, for every max_hits around
    the rounds of 8 and 16 steps; two toeholds wrapped below zero.  Locations: Oracle.locs_at_batch (toehold_sa.hpp:37-49)."""
    rb, R = handles(form), ref
    N = n
    pos_bytes = form[1]
    for mh in MAX_HITS:
        c = Case(R, 1)     # (the reads themselves are not used: ranges and toeholds in, locations out)
        L, st = c.L, c.st
        woff, wlocs = R.locs[mh]
        woff = woff[:N + 1]
        total = int(woff[N])
        wlocs = wlocs[:total]
        lo, hi, k = c.inp("d_lo", R.lo[:N]), c.inp("d_hi", R.hi[:N]), c.inp("d_k", R.k[:N])
        tmp_bytes, ws_bytes = int(L.rbg_locate_plan_tmp_bytes(N)), int(L.rbg_locate_order_ws_bytes(N))
        loc_off = c.u64("d_loc_off", N + 1)
        tmp = c.out("d_tmp", tmp_bytes, 8)
        ws = c.out("d_order_ws", ws_bytes, 256)
        c.freeze()
        assert L.rbg_locate_plan_dev(rb.h, lo.ptr, hi.ptr, N, mh, loc_off.ptr, tmp.ptr, tmp_bytes, st) == 0
        assert L.rbg_locate_order_dev(rb.h, k.ptr, N, ws.ptr, ws_bytes, st) == 0
        c.sync_and_check()
        same(loc_off, woff)
        c.freeze("d_loc_off", "d_order_ws")
        outs = []
        for skew in (8, 56):
            for order in (None, ws.ptr):
                d = c.u64(f"d_locs_{skew}_{'ordered' if order else 'plain'}", total, skew=skew)
                assert L.rbg_locate_fill_dev(rb.h, lo.ptr, hi.ptr, k.ptr, N, mh, loc_off.ptr, d.ptr, order, st) == 0
                outs.append(d)
        d32 = [c.out(f"d_locs32_{'ordered' if order else 'plain'}", 4 * total, 4) for order in (None, ws.ptr)]
        for d, order in zip(d32, (None, ws.ptr)):
            rc = L.rbg_locate_fill_dev32(rb.h, lo.ptr, hi.ptr, k.ptr, N, mh, loc_off.ptr, d.ptr, order, st)
            assert rc == (0 if pos_bytes == 4 else EARG)
        c.sync_and_check()
        for d in outs:
            same(d, wlocs)
        for d in d32:
            if pos_bytes == 4:
                same(d, (wlocs & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.uint32)
            else:
                c.A.check_untouched(d.name, [(0, d.nbytes)])     # refused: nothing written


@forms
@cases
def test_locate_refusals(ref, handles, form, n):
    """undersized declarations of the locate plan's scratch and the order workspace (size - 1 and 0), the order workspace at 128-byte alignment: RBG_EARG,
    and not a byte of the arena changes -- the plan's launcher used to zero d_loc_off[0] before it looked at tmp_bytes"""
    rb, R = handles(form), ref
    N = n
    c = Case(R, 1)
    L, st = c.L, c.st
    lo, hi, k = c.inp("d_lo", R.lo[:N]), c.inp("d_hi", R.hi[:N]), c.inp("d_k", R.k[:N])
    tmp_bytes, ws_bytes = int(L.rbg_locate_plan_tmp_bytes(N)), int(L.rbg_locate_order_ws_bytes(N))
    loc_off, mk_off = c.u64("d_loc_off", N + 1), c.u64("d_mk_off", N + 1)
    tmp = c.out("d_tmp", tmp_bytes, 8)
    ws = c.out("d_order_ws", ws_bytes + 128, 256)
    before = c.A.buf.clone()
    for declared in (tmp_bytes - 1, 0):
        assert L.rbg_locate_plan_dev(rb.h, lo.ptr, hi.ptr, N, MAXU, loc_off.ptr, tmp.ptr, declared, st) == EARG
        assert L.rbg_markers_plan_dev(rb.h, lo.ptr, hi.ptr, N, mk_off.ptr, tmp.ptr, declared, st) == EARG
    for declared in (ws_bytes - 1, 0):
        assert L.rbg_locate_order_dev(rb.h, k.ptr, N, ws.ptr, declared, st) == EARG
    assert L.rbg_locate_order_dev(rb.h, k.ptr, N, ws.ptr + 128, ws_bytes, st) == EARG       # (full memory behind it, 128-byte alignment)
    c.torch.cuda.synchronize()
    assert bool((c.A.buf == before).all().item())


# ---- markers of a range -----------------------------------------------------------------------------------------------------------------------------
@forms
@cases
def test_markers(ref, handles, form, n):
    """rbg_markers_plan_dev / rbg_markers_fill_dev against Oracle.markers_at (MarkerArray::at_range)"""
    rb, R = handles(form), ref
    N = n
    c = Case(R, 1)
    L, st = c.L, c.st
    lo, hi = c.inp("d_lo", R.lo[:N]), c.inp("d_hi", R.hi[:N])
    tmp_bytes = int(L.rbg_locate_plan_tmp_bytes(N))
    mk_off, tmp = c.u64("d_mk_off", N + 1), c.out("d_tmp", tmp_bytes, 8)
    c.freeze()
    assert L.rbg_markers_plan_dev(rb.h, lo.ptr, hi.ptr, N, mk_off.ptr, tmp.ptr, tmp_bytes, st) == 0
    c.sync_and_check()
    want = R.markers_at[:N]
    woff = scan([len(w) for w in want])
    same(mk_off, woff)
    c.freeze("d_mk_off")
    mk = c.u64("d_mk", int(woff[N]))
    assert L.rbg_markers_fill_dev(rb.h, lo.ptr, hi.ptr, N, mk_off.ptr, mk.ptr, st) == 0
    c.sync_and_check()
    same(mk, [v for w in want for v in w])


# ---- marker seeds, with and without the log --------------------------------------------------------------------------------------------------------
def _check_seed_records(recs, mk, mk_off, seed_off, want, rec_base=None):
    """records [lo, hi, qstart, qend, mk_begin, mk_end] of every read against the reference's (lo, hi, qstart, qend, markers): a record's markers are
    mk[mk_begin, mk_end), they lie in the read's own stretch of mk and together fill it"""
    for i, w in enumerate(want):
        a = int(seed_off[i]) if rec_base is None else int(rec_base[i])
        used = 0
        for t, (wl, wh, wqs, wqe, wm) in enumerate(w):
            g = [int(x) for x in recs[a + t]]
            assert g[:4] == [wl, wh, wqs, wqe], (i, t, g)
            assert int(mk_off[i]) <= g[4] <= g[5] <= int(mk_off[i + 1]), (i, t, g)
            assert mk[g[4]:g[5]].tolist() == wm, (i, t)
            used += g[5] - g[4]
        assert used == int(mk_off[i + 1] - mk_off[i]), i


@forms
@cases
def test_marker_seeds(ref, handles, form, n):
    """rbg_marker_seeds_plan_dev / _fill_dev, and the _log pair with a log of exactly rbg_marker_seeds_log_bytes for a quota of 1 (most reads overflow
    into the list at the log's end) and of 12: get_markers_greedy_seeding (rowbowt.hpp:406-482) from the oracle.  The log declared one byte short: RBG_EARG."""
    rb, R = handles(form), ref
    N = n
    want = R.marker_seeds[:N]
    wsoff = scan([len(w) for w in want])
    wmoff = scan([sum(len(r[4]) for r in w) for w in want])
    ns, nm = int(wsoff[N]), int(wmoff[N])
    c = Case(R, N)
    L, st = c.L, c.st
    seqs, off = c.seqs.ptr, c.off.ptr
    tmp_bytes = int(L.rbg_locate_plan_tmp_bytes(N))
    tmp = c.out("d_tmp", tmp_bytes, 8)
    c.freeze()
    runs = []
    for tag, quota in (("walk", None), ("log1", 1), ("log12", 12)):
        soff, moff = c.u64(f"d_seed_off_{tag}", N + 1), c.u64(f"d_mk_off_{tag}", N + 1)
        seeds = c.out(f"d_seeds_{tag}", 48 * ns, 8 if quota is None else 16)
        mk = c.u64(f"d_mk_{tag}", nm)
        mkp = mk.ptr if nm else None
        if quota is None:
            assert L.rbg_marker_seeds_plan_dev(rb.h, seqs, off, N, WSIZE, MAX_RANGE, 0, soff.ptr, moff.ptr, tmp.ptr, tmp_bytes, st) == 0
            assert L.rbg_marker_seeds_fill_dev(rb.h, seqs, off, N, WSIZE, MAX_RANGE, 0, soff.ptr, moff.ptr, seeds.ptr, mkp, st) == 0
        else:
            log_bytes = int(L.rbg_marker_seeds_log_bytes(rb.h, N, quota))
            log = c.out(f"d_log_{tag}", log_bytes, 16)
            if quota == 1:
                before = c.A.buf.clone()
                assert L.rbg_marker_seeds_plan_log_dev(rb.h, seqs, off, N, WSIZE, MAX_RANGE, 0, soff.ptr, moff.ptr, tmp.ptr, tmp_bytes, log.ptr, log_bytes - 1, st) == EARG
                assert L.rbg_marker_seeds_fill_log_dev(rb.h, seqs, off, N, WSIZE, MAX_RANGE, 0, soff.ptr, moff.ptr, seeds.ptr, mkp, log.ptr, log_bytes - 1, st) == EARG
                for declared in (tmp_bytes - 1, 0):
                    assert L.rbg_marker_seeds_plan_dev(rb.h, seqs, off, N, WSIZE, MAX_RANGE, 0, soff.ptr, moff.ptr, tmp.ptr, declared, st) == EARG
                    assert L.rbg_marker_seeds_plan_log_dev(rb.h, seqs, off, N, WSIZE, MAX_RANGE, 0, soff.ptr, moff.ptr, tmp.ptr, declared, log.ptr, log_bytes, st) == EARG
                c.torch.cuda.synchronize()
                assert bool((c.A.buf == before).all().item())
            assert L.rbg_marker_seeds_plan_log_dev(rb.h, seqs, off, N, WSIZE, MAX_RANGE, 0, soff.ptr, moff.ptr, tmp.ptr, tmp_bytes, log.ptr, log_bytes, st) == 0
            assert L.rbg_marker_seeds_fill_log_dev(rb.h, seqs, off, N, WSIZE, MAX_RANGE, 0, soff.ptr, moff.ptr, seeds.ptr, mkp, log.ptr, log_bytes, st) == 0
        runs.append((soff, moff, seeds, mk))
    c.sync_and_check()
    for soff, moff, seeds, mk in runs:
        same(soff, wsoff)
        same(moff, wmoff)
        _check_seed_records(seeds.numpy(np.uint64).reshape(ns, 6), mk.numpy(np.uint64), wmoff, wsoff, want)


@forms
@cases
def test_marker_lmems(ref, handles, form, n):
    """rbg_marker_lmems_plan_dev / _fill_dev with d_off[0] = 32 (garbage before the first read), d_mk NULL when the plan says 0: get_markers_lmems
    (rowbowt.hpp:341-404) from tests/lmem_model.py; the scratch declared one byte short and empty: RBG_EARG"""
    rb, R = handles(form), ref
    N = n
    want = R.lmems[:N]
    c = Case(R, N, pad_byte=0x4E, lead=32)
    L, st = c.L, c.st
    seqs, off = c.seqs.ptr, c.off.ptr
    total = c.total
    tmp_bytes = int(L.rbg_marker_lmems_tmp_bytes(N, total))
    tmp = c.out("d_tmp", tmp_bytes, 8)
    mk_off = c.u64("d_mk_off", N + 1)
    c.freeze()
    before = c.A.buf.clone()
    for declared in (tmp_bytes - 1, 0):
        assert L.rbg_marker_lmems_plan_dev(rb.h, seqs, off, N, total, WSIZE, MAX_RANGE, 0, mk_off.ptr, tmp.ptr, declared, st) == EARG
    c.torch.cuda.synchronize()
    assert bool((c.A.buf == before).all().item())
    assert L.rbg_marker_lmems_plan_dev(rb.h, seqs, off, N, total, WSIZE, MAX_RANGE, 0, mk_off.ptr, tmp.ptr, tmp_bytes, st) == 0
    c.sync_and_check()
    wmoff = scan([sum(len(r[4]) for r in w) for w in want])
    same(mk_off, wmoff)
    nm = int(wmoff[N])
    c.freeze("d_tmp")
    seeds, mk = c.out("d_seeds", 48 * total, 8), c.u64("d_mk", nm)
    assert L.rbg_marker_lmems_fill_dev(rb.h, seqs, off, N, total, WSIZE, MAX_RANGE, 0, tmp.ptr, seeds.ptr, mk.ptr if nm else None, st) == 0
    c.sync_and_check()
    assert all(len(w) == len(q) for w, q in zip(want, R.reads[:N]))
    _check_seed_records(seeds.numpy(np.uint64).reshape(total, 6), mk.numpy(np.uint64), wmoff, None, want, rec_base=R.off[:N])


# ---- greedy seed lists, and the locations of every seed ------------------------------------------------------------------------------------------------
@forms
@cases
@pytest.mark.parametrize("w_sample", [True, False])
def test_greedy_seeds(ref, handles, form, n, w_sample):
    """rbg_greedy_seeds_plan_dev / _fill_dev with and without RBG_SEEDS_W_SAMPLE (d_ssamp NULL without it) against tests/seeds_model.py; with the sample
    the arrays go on into rbg_locate_plan_dev and rbg_locate_fill_offset_dev (d_sub = d_qstart): Oracle.locs_at minus qstart for every seed"""
    rb, R = handles(form), ref
    N = n
    flags = capi.SEEDS_W_SAMPLE if w_sample else 0
    want = R.seed_lists[w_sample][:N]
    wsoff = scan([len(w) for w in want])
    ns = int(wsoff[N])
    c = Case(R, N)
    L, st = c.L, c.st
    seqs, off = c.seqs.ptr, c.off.ptr
    tmp_bytes = int(L.rbg_greedy_seeds_tmp_bytes(N))
    tmp, soff = c.out("d_tmp", tmp_bytes, 8), c.u64("d_seed_off", N + 1)
    c.freeze()
    before = c.A.buf.clone()
    for declared in (tmp_bytes - 1, 0):
        assert L.rbg_greedy_seeds_plan_dev(rb.h, seqs, off, N, MIN_LENGTH, flags, soff.ptr, tmp.ptr, declared, st) == EARG
    c.torch.cuda.synchronize()
    assert bool((c.A.buf == before).all().item())
    assert L.rbg_greedy_seeds_plan_dev(rb.h, seqs, off, N, MIN_LENGTH, flags, soff.ptr, tmp.ptr, tmp_bytes, st) == 0
    c.sync_and_check()
    same(soff, wsoff)
    c.freeze("d_seed_off")
    cols = [c.u64("d_s_" + f, ns) for f in ("lo", "hi", "qstart", "qend")]
    ss = c.u64("d_s_ssamp", ns) if w_sample else None
    assert L.rbg_greedy_seeds_fill_dev(rb.h, seqs, off, N, MIN_LENGTH, flags, soff.ptr, *(t.ptr for t in cols), ss.ptr if ss else None, st) == 0
    c.sync_and_check()
    flat = [r for w in want for r in w]
    for j, t in enumerate(cols):
        same(t, [r[j] for r in flat])
    if not w_sample or ns == 0:
        return
    same(ss, [r[4] for r in flat])
    # locate every seed
    mh = 7
    wlo, whi, wqs, wss = (np.array([r[j] for r in flat], np.uint64) for j in (0, 1, 2, 4))
    woff, wlocs = R.o.locs_at_batch(wlo, whi, wss, mh, nthreads=4)
    with np.errstate(over="ignore"):
        wlocs = wlocs - np.repeat(wqs, np.diff(woff).astype(np.int64))
    c.freeze("d_s_lo", "d_s_hi", "d_s_qstart", "d_s_ssamp")
    ltmp_bytes = int(L.rbg_locate_plan_tmp_bytes(ns))
    ltmp, loff = c.out("d_ltmp", ltmp_bytes, 8), c.u64("d_loc_off", ns + 1)
    assert L.rbg_locate_plan_dev(rb.h, cols[0].ptr, cols[1].ptr, ns, mh, loff.ptr, ltmp.ptr, ltmp_bytes, st) == 0
    c.sync_and_check()
    same(loff, woff)
    c.freeze("d_loc_off")
    locs = c.u64("d_locs", int(woff[ns]))
    assert L.rbg_locate_fill_offset_dev(rb.h, cols[0].ptr, cols[1].ptr, ss.ptr, ns, mh, loff.ptr, locs.ptr, cols[2].ptr, None, st) == 0
    c.sync_and_check()
    same(locs, wlocs)


# ---- toehold checkpoints in fixed slots -----------------------------------------------------------------------------------------------------------------
@forms
@cases
def test_toehold_chkpnts(ref, handles, form, n):
    """rbg_toehold_chkpnts_slots_dev and rbg_find_range_w_toehold_chkpnts_dev (rowbowt.hpp:575-606, tests/seeds_model.py): the slots of a read with
    d_cnt == 0 are unspecified, everything outside every read's slots -- the arrays hold nothing but slots -- is untouched"""
    rb, R = handles(form), ref
    N = n
    want = R.chkpnts[:N]
    wslot = scan([chkpnt_count(len(q), CHK_WSIZE) for q in R.reads[:N]])
    S = int(wslot[N])
    c = Case(R, N)
    L, st = c.L, c.st
    seqs, off = c.seqs.ptr, c.off.ptr
    tmp_bytes = int(L.rbg_toehold_chkpnts_tmp_bytes(N))
    tmp, slot_off = c.out("d_tmp", tmp_bytes, 8), c.u64("d_slot_off", N + 1)
    c.freeze()
    before = c.A.buf.clone()
    for declared in (tmp_bytes - 1, 0):
        assert L.rbg_toehold_chkpnts_slots_dev(rb.h, off, N, CHK_WSIZE, slot_off.ptr, tmp.ptr, declared, st) == EARG
    c.torch.cuda.synchronize()
    assert bool((c.A.buf == before).all().item())
    assert L.rbg_toehold_chkpnts_slots_dev(rb.h, off, N, CHK_WSIZE, slot_off.ptr, tmp.ptr, tmp_bytes, st) == 0
    c.sync_and_check()
    same(slot_off, wslot)
    c.freeze("d_slot_off")
    cnt = c.u64("d_cnt", N)
    cols = [c.u64("d_c_" + f, S) for f in ("lo", "hi", "qstart", "qend", "ssamp")]
    assert L.rbg_find_range_w_toehold_chkpnts_dev(rb.h, seqs, off, N, CHK_WSIZE, slot_off.ptr, cnt.ptr, *(t.ptr for t in cols), st) == 0
    c.sync_and_check()
    same(cnt, [len(w) for w in want])
    got = [t.numpy(np.uint64) for t in cols]
    for i, w in enumerate(want):
        assert len(w) in (0, int(wslot[i + 1] - wslot[i])), i
        s = int(wslot[i])
        assert [tuple(int(g[s + t]) for g in got) for t in range(len(w))] == w, i


# ---- markers at located text positions --------------------------------------------------------------------------------------------------------------------
@forms
@cases
@pytest.mark.parametrize("group", [4, 16, 64])
def test_loc_markers(ref, handles, form, n, group):
    """rbg_loc_markers_plan_dev / _fill_dev over the oracle's locations (two of them wrapped below zero), RBG_LOCMK_GROUP forced: tests/rb_locs_model.py"""
    rb, R = handles(form), ref
    N = n
    woff, wlocs = R.locs[LOCMK_HITS]
    woff = woff[:N + 1]
    wlocs = wlocs[:int(woff[N])]
    want = R.loc_markers[:N]
    wmoff = scan([len(w) for w in want])
    c = Case(R, N)
    L, st = c.L, c.st
    locs, loc_off = c.inp("d_locs", wlocs), c.inp("d_loc_off", woff)
    tmp_bytes = int(L.rbg_loc_markers_tmp_bytes(N))
    tmp, mk_off = c.out("d_tmp", tmp_bytes, 8), c.u64("d_mk_off", N + 1)
    mk = c.u64("d_mk", int(wmoff[N]))
    c.freeze()
    lp = locs.ptr      # (an empty location list still gets an address inside the arena)
    with env("RBG_LOCMK_GROUP", group):
        before = c.A.buf.clone()
        for declared in (tmp_bytes - 1, 0):
            assert L.rbg_loc_markers_plan_dev(rb.h, lp, loc_off.ptr, c.off.ptr, N, mk_off.ptr, tmp.ptr, declared, st) == EARG
        c.torch.cuda.synchronize()
        assert bool((c.A.buf == before).all().item())
        assert L.rbg_loc_markers_plan_dev(rb.h, lp, loc_off.ptr, c.off.ptr, N, mk_off.ptr, tmp.ptr, tmp_bytes, st) == 0
        c.sync_and_check()
        same(mk_off, wmoff)
        c.freeze("d_mk_off")
        assert L.rbg_loc_markers_fill_dev(rb.h, lp, loc_off.ptr, c.off.ptr, N, mk_off.ptr, mk.ptr, st) == 0
        c.sync_and_check()
    same(mk, [v for w in want for v in w])


# ---- the strands of the report -----------------------------------------------------------------------------------------------------------------------
@forms
@cases
def test_read_strands(ref, handles, form, n):
    """rbg_read_strands_dev with d_off[0] = 48 and d_seqs2 of exactly rbg_read_strands_bytes: seq_ntoa_table and the reverse complement
    (rb_markers.cpp:139-156, tests/rb_markers_model.py)"""
    rb, R = handles(form), ref
    N = n
    c = Case(R, N, pad_byte=0x07, lead=48)
    L, st = c.L, c.st
    total = c.total
    nbytes = int(L.rbg_read_strands_bytes(total))
    seqs2, off2 = c.out("d_seqs2", nbytes, 16), c.u64("d_off2", 2 * N + 1)
    c.freeze()
    assert L.rbg_read_strands_dev(rb.h, c.seqs.ptr, c.off.ptr, N, total, seqs2.ptr, off2.ptr, st) == 0
    c.sync_and_check()
    want, woff = b"", [0]
    for q in R.reads[:N]:
        fwd = q.translate(RM.NT)
        want += fwd + fwd.translate(RM.COMP)[::-1]
        woff += [woff[-1] + len(q), woff[-1] + 2 * len(q)]
    same(off2, woff)
    assert seqs2.numpy().tobytes()[:2 * total] == want
    c.A.check_untouched("d_seqs2", [(up16(2 * total), nbytes)])     # nothing beyond the last 16-byte piece
    refused(c, (L.rbg_read_strands_dev, rb.h, c.seqs.ptr, c.off.ptr, N, total, seqs2.ptr + 8, off2.ptr, st),
            (L.rbg_read_strands_dev, rb.h, c.seqs.ptr + 8, c.off.ptr, N, total, seqs2.ptr, off2.ptr, st))


# ---- documents ------------------------------------------------------------------------------------------------------------------------------------------
def _doc_outputs(c, tag, N, W, nd, with_locs=False):
    o = {"sets": c.u64(f"d_sets_{tag}", N * W), "ndocs": c.out(f"d_ndocs_{tag}", 4 * N, 4), "nodoc": c.out(f"d_nodoc_{tag}", 4 * N, 4),
         "doc_reads": c.u64(f"d_doc_reads_{tag}", nd)}
    o["doc_reads"].fill_from(np.arange(1000, 1000 + nd, dtype=np.uint64))      # accumulating arrays: distinct non-zero values
    if with_locs:
        o["doc_locs"] = c.u64(f"d_doc_locs_{tag}", nd)
        o["doc_locs"].fill_from(np.arange(5000, 5000 + 3 * nd, 3, dtype=np.uint64))
    return o


def _check_doc_outputs(c, o, want, skip=None, doc_locs=None):
    sets, ndocs, nodoc, doc_reads = want
    nd = len(doc_reads)
    for key, w, dt in (("sets", sets.reshape(-1), np.uint64), ("ndocs", ndocs, np.uint32), ("nodoc", nodoc, np.uint32),
                       ("doc_reads", doc_reads + np.arange(1000, 1000 + nd, dtype=np.uint64), np.uint64)):
        if key == skip:
            if key == "doc_reads":
                same(o[key], np.arange(1000, 1000 + nd, dtype=np.uint64))
            else:
                c.A.check_untouched(o[key].name, [(0, o[key].nbytes)])
        else:
            same(o[key], w, dt)
    if "doc_locs" in o:
        base = np.arange(5000, 5000 + 3 * nd, 3, dtype=np.uint64)
        same(o["doc_locs"], base if skip == "doc_locs" else base + doc_locs)


@forms
@cases
def test_documents(ref, handles, form, n):
    """rbg_resolve_offsets_dev[32] (d_offset NULL and not), rbg_doc_hits_dev[32] and rbg_locate_doc_hits_dev with every nullable output NULL in turn and
    RBG_DOCS_GROUP forced to 4, 16 and 64, the accumulating arrays pre-filled with distinct values; 70 documents (a row of d_sets ends inside a word):
    tests/doc_hits_model.py (DocList::doc_and_offset_at, doclist.hpp:46-50, :77-79)"""
    rb, R = handles(form), ref
    N, nd = n, NDOCS
    W = (nd + 63) // 64
    assert int(ra.lib().rbg_doc_hits_words(rb.h)) == W == 2
    mh = 17
    woff, wlocs = R.locs[mh]
    woff = woff[:N + 1]
    M = int(woff[N])
    wlocs = wlocs[:M]
    l32 = np.where(wlocs == np.uint64(MAXU), np.uint64(0xFFFFFFFF), wlocs & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    wide = DM.widen32(l32)
    c = Case(R, 1)
    L, st = c.L, c.st
    locs, locs32, loc_off = c.inp("d_locs", wlocs), c.inp("d_locs32", l32, 4), c.inp("d_loc_off", woff)
    lo, hi, k = c.inp("d_lo", R.lo[:N]), c.inp("d_hi", R.hi[:N]), c.inp("d_k", R.k[:N])
    c.freeze()
    # resolve
    res = []
    for tag, src, fn, wl in (("64", locs, L.rbg_resolve_offsets_dev, wlocs), ("32", locs32, L.rbg_resolve_offsets_dev32, wide)):
        for with_off in (True, False):
            d_doc = c.out(f"d_doc_{tag}_{int(with_off)}", 4 * M, 4)
            d_o = c.u64(f"d_offset_{tag}_{int(with_off)}", M)
            assert fn(rb.h, src.ptr, M, d_doc.ptr, d_o.ptr if with_off else None, st) == 0
            res.append((d_doc, d_o, with_off, wl))
    c.sync_and_check()
    for d_doc, d_o, with_off, wl in res:
        wdoc, woffs = DM.resolve(wl, R.doc_starts)
        same(d_doc, wdoc, np.uint32)
        if with_off:
            same(d_o, woffs)
        else:
            c.A.check_untouched(d_o.name, [(0, d_o.nbytes)])
    # hits over stored locations
    want = DM.doc_hits(wlocs, woff, R.doc_starts)
    want32 = DM.doc_hits(wide, woff, R.doc_starts)
    runs = []
    for group in (4, 16, 64):
        with env("RBG_DOCS_GROUP", group):
            for tag, src, fn, w in (("64", locs, L.rbg_doc_hits_dev, want), ("32", locs32, L.rbg_doc_hits_dev32, want32)):
                for skip in ((None, "sets", "ndocs", "nodoc", "doc_reads") if group == 16 else (None,)):
                    o = _doc_outputs(c, f"{tag}_g{group}_{skip}", N, W, nd)
                    p = {key: (None if key == skip else t.ptr) for key, t in o.items()}
                    assert fn(rb.h, src.ptr, loc_off.ptr, N, p["sets"], p["ndocs"], p["nodoc"], p["doc_reads"], st) == 0
                    runs.append((o, w, skip, None))
    # the fused walk: no locations stored
    order_bytes = int(L.rbg_locate_order_ws_bytes(N))
    ws = c.out("d_order_ws", order_bytes, 256)
    assert L.rbg_locate_order_dev(rb.h, k.ptr, N, ws.ptr, order_bytes, st) == 0
    wdoc, _ = DM.resolve(wlocs, R.doc_starts)
    doc_locs = np.bincount(wdoc[wdoc != DM.DOC_NONE].astype(np.int64), minlength=nd).astype(np.uint64)
    for order in (None, ws.ptr):
        for skip in (None, "sets", "ndocs", "nodoc", "doc_reads", "doc_locs") if order is None else (None,):
            o = _doc_outputs(c, f"fused_{'ordered' if order else 'plain'}_{skip}", N, W, nd, with_locs=True)
            p = {key: (None if key == skip else t.ptr) for key, t in o.items()}
            assert L.rbg_locate_doc_hits_dev(rb.h, lo.ptr, hi.ptr, k.ptr, N, mh, order, p["sets"], p["ndocs"], p["nodoc"], p["doc_reads"], p["doc_locs"], st) == 0
            runs.append((o, want, skip, doc_locs))
    c.sync_and_check()
    for o, w, skip, dl in runs:
        _check_doc_outputs(c, o, w, skip, dl)


# ---- the tally's scratch ------------------------------------------------------------------------------------------------------------------------------
@forms
def test_tally_refusals(ref, handles, form):
    """rbg_tally_add_dev and rbg_tally_add_reads_dev with their scratch declared one byte short and empty: RBG_EARG, nothing in the arena changes"""
    rb, R = handles(form), ref
    import ctypes
    c = Case(R, 1)
    L, st = c.L, c.st
    Rn, Nn = 5, 3
    recs = c.inp("d_recs", np.zeros(Rn * 6, np.uint64))          # (five records without markers)
    rep_off = c.inp("d_rep_off", np.array([0, 2, 2, 5], np.uint64))
    mk = c.inp("d_mk", np.zeros(4, np.uint64))
    t = capi.VP()
    assert L.rbg_tally_create(rb.h, 64, ctypes.byref(t)) == 0
    try:
        b1, b2 = int(L.rbg_tally_add_tmp_bytes(Rn)), int(L.rbg_tally_add_reads_tmp_bytes(Nn, Rn))
        tmp = c.out("d_tmp", max(b1, b2), 8)
        before = c.A.buf.clone()
        for declared in (b1 - 1, 0):
            assert L.rbg_tally_add_dev(t, recs.ptr, Rn, mk.ptr, 0, tmp.ptr, declared, st) == EARG
        for declared in (b2 - 1, 0):
            assert L.rbg_tally_add_reads_dev(t, recs.ptr, Rn, rep_off.ptr, Nn, mk.ptr, 0, 1, tmp.ptr, declared, st) == EARG
        c.torch.cuda.synchronize()
        assert bool((c.A.buf == before).all().item())
    finally:
        L.rbg_tally_free(t)


# ---- the report: canon in place, then select ---------------------------------------------------------------------------------------------------------
M64 = MAXU
CANON_FLAGS = {4: 0, 16: capi.REPORT_CLEAR_CONFLICTING | capi.REPORT_CLEAR_IDENTICAL, 64: capi.REPORT_CLEAR_IDENTICAL}
CANON_MIN_RANGE, REPORT_READ_LEN = 2, 101


def _canon_want(s, lo, hi, min_range, read_len, flags):
    """one record's markers after rbg_marker_seeds_canon_dev (rb_markers.cpp:374-380, :266-284, through tests/rb_markers_model.py)"""
    ms = sorted(set(s), key=RM.marker_key) if ((hi - lo + 1) & M64) >= min_range and s else []
    if flags & capi.REPORT_CLEAR_CONFLICTING:
        ms = RM.clear_if_conflicting(ms, read_len)
    if flags & capi.REPORT_CLEAR_IDENTICAL:
        ms = RM.filter_identical_pos(ms)
    return ms


def _select_model(by_seq, lens, coins, heuristic, best_strand, min_seed_len, read_len):
    """rbg_report_select_dev from the records of the 2N sequences (sequence 2i = read i forward, 2i + 1 = its reverse complement), each (lo, hi, qstart,
    qend, mk_begin, mk_end): worker and worker_heuristic of rb_markers.cpp as tests/rb_markers_model.py's expected_stdout states them, record for record
    -> (rep_off, [(range_size, query_start, query_len, mk_begin, mk_end, strand)], the read of every record)"""
    out, reads, rep_off = [], [], [0]
    for i, n in enumerate(lens):
        seeds = []

        def run(j, strand):
            stop = False
            for lo, hi, qs, qe, b, e in by_seq[j]:
                range_size = (hi - lo + 1) & M64
                qstart = ((n - qs - 1) & M64) if strand else qs
                qlen = (qe - qs) & M64
                if hi < lo or (heuristic and qlen < min_seed_len):
                    continue
                seeds.append((range_size, qstart, qlen, b, e, strand))
                if heuristic and best_strand and ((read_len - (qstart + qlen)) & M64) < min_seed_len:
                    stop = True
            return stop

        if not heuristic:
            run(2 * i, 0)
            run(2 * i + 1, 1)
        else:
            first_fwd = True if coins is None else bool(coins[i])
            one, two = ((2 * i, 0), (2 * i + 1, 1)) if first_fwd else ((2 * i + 1, 1), (2 * i, 0))
            if not run(*one):
                run(*two)
            if best_strand and seeds:
                best = max(range(len(seeds)), key=lambda t: (seeds[t][2], -t))
                seeds = [s for s in seeds if s[5] == seeds[best][5]]
            if min_seed_len:
                seeds = [s for s in seeds if s[2] >= min_seed_len]
        out += seeds
        reads += [i] * len(seeds)
        rep_off.append(len(out))
    return np.array(rep_off, np.uint64), out, np.array(reads, np.uint32)


def _check_selected(c, rep_off, d_out, d_out_read, want, cap_records):
    w_off, w_recs, w_reads = want
    same(rep_off, w_off)
    R = len(w_recs)
    got = d_out.numpy().view(capi.REPORT_SEED)
    for f, j in (("range_size", 0), ("query_start", 1), ("query_len", 2), ("mk_begin", 3), ("mk_end", 4), ("strand", 5)):
        assert got[f][:R].tolist() == [r[j] for r in w_recs], f
    c.A.check_untouched(d_out.name, [(48 * R, 48 * cap_records)])              # room for every input record; nothing behind the printed ones
    if d_out_read is not None:
        assert d_out_read.numpy(np.uint32)[:R].tolist() == w_reads.tolist()
        c.A.check_untouched(d_out_read.name, [(4 * R, 4 * cap_records)])


@pytest.fixture(scope="module")
def report_ref(ref):
    """the seed records of both strands of every read from the oracle (get_markers_greedy_seeding), their markers dense in record order as the fills leave
    them, and behind sentinel words two records of no read that are long enough for the workgroup path (300 markers) and its chunked form (5000)"""
    R = ref
    rng = np.random.default_rng(23)
    by_seq = []
    for q in R.reads:
        fwd = q.translate(RM.NT)
        for s in (fwd, fwd.translate(RM.COMP)[::-1]):
            by_seq.append(R.o.markers_greedy_seeding(s, WSIZE, MAX_RANGE, 0))
    pool = [int(v) for v in R.markers[3][:40]]
    longs = []
    for n in (300, 5000):
        longs.append([pool[int(t)] for t in rng.integers(0, len(pool), n // 2)] + [int(v) for v in rng.integers(0, 2**63, n - n // 2, dtype=np.uint64) * 2 + 1])
    assert sum(1 for w in by_seq for r in w if len(r[4]) > 1) > 50
    return by_seq, longs


@forms
@cases
def test_report_canon_and_select(ref, report_ref, handles, form, n):
    """rbg_marker_seeds_canon_dev in place with RBG_REPORT_GROUP forced to 4, 16 and 64 (another filter set each), its scratch at 4-byte alignment and of
    exact size: every record's survivors are the model's, mk_end = mk_begin + their number, and every byte of d_mk outside [mk_begin, old mk_end) of every
    record -- the sentinel words included -- is what it was; the first five words of every record too.  Then rbg_report_select_dev over the canonical
    records (carved from the model's, not from the run before) in default and in heuristic mode with coins, with and without d_out_read.  Both calls with
    their scratch declared one byte short and empty: RBG_EARG."""
    rb, R = handles(form), ref
    N = n
    by_seq, longs = report_ref
    by_seq = by_seq[:2 * N]
    recs, mk, seed_off = [], [], [0]
    for w in by_seq:
        for lo, hi, qs, qe, m in w:
            recs.append([lo, hi, qs, qe, len(mk), len(mk) + len(m)])
            mk += m
        seed_off.append(len(recs))
    S_reads = len(recs)
    for j, s in enumerate(longs):
        mk += [0xDEADBEEF00000000 + len(mk) + t for t in range(3)]
        recs.append([10, 12 + j, 5, 25, len(mk), len(mk) + len(s)])
        mk += s
    mk += [0xDEADBEEF00000000 + len(mk) + t for t in range(3)]
    S = len(recs)
    h_recs, h_mk = np.array(recs, np.uint64).reshape(S, 6), np.array(mk, np.uint64)
    c = Case(R, 1)
    L, st = c.L, c.st
    tmp_bytes = int(L.rbg_marker_seeds_canon_tmp_bytes(S))
    tmp = c.out("d_canon_tmp", tmp_bytes, 4)
    runs = []
    for group, flags in CANON_FLAGS.items():
        d_seeds, d_mk = c.A.carve_from(f"d_seeds_g{group}", h_recs, 8), c.A.carve_from(f"d_mk_g{group}", h_mk, 8)
        runs.append((group, flags, d_seeds, d_mk))
    c.freeze()
    refused(c, *[(L.rbg_marker_seeds_canon_dev, rb.h, runs[0][2].ptr, S, runs[0][3].ptr, CANON_MIN_RANGE, 0, REPORT_READ_LEN, tmp.ptr, declared, st)
                 for declared in (tmp_bytes - 1, 0)],
            (L.rbg_marker_seeds_canon_dev, rb.h, runs[0][2].ptr, S, runs[0][3].ptr, CANON_MIN_RANGE, 0, REPORT_READ_LEN, tmp.ptr + 2, tmp_bytes, st))
    for group, flags, d_seeds, d_mk in runs:
        with env("RBG_REPORT_GROUP", group):
            assert L.rbg_marker_seeds_canon_dev(rb.h, d_seeds.ptr, S, d_mk.ptr, CANON_MIN_RANGE, flags, REPORT_READ_LEN, tmp.ptr, tmp_bytes, st) == 0
    c.sync_and_check()
    canon = {}
    for group, flags, d_seeds, d_mk in runs:
        g_recs, g_mk = d_seeds.numpy(np.uint64).reshape(S, 6), d_mk.numpy(np.uint64)
        assert (g_recs[:, :5] == h_recs[:, :5]).all(), group
        keep = np.ones(len(h_mk), bool)
        out = []
        for j in range(S):
            b, e_old = int(h_recs[j, 4]), int(h_recs[j, 5])
            keep[b:e_old] = False
            want = _canon_want(mk[b:e_old], int(h_recs[j, 0]), int(h_recs[j, 1]), CANON_MIN_RANGE, REPORT_READ_LEN, flags)
            assert int(g_recs[j, 5]) == b + len(want) and g_mk[b:b + len(want)].tolist() == want, (group, j)
            out.append([int(v) for v in h_recs[j, :4]] + [b, b + len(want)])
        assert (g_mk[keep] == h_mk[keep]).all() and int(keep.sum()) == 9, group     # no other byte of d_mk is written
        canon[group] = out
    assert sum(r[5] - r[4] for r in canon[4]) > sum(r[5] - r[4] for r in canon[16])
    # select, over the model's canonical records of the reads (the two long records belong to no read)
    sel_recs = canon[4][:S_reads]
    sel_by_seq = [sel_recs[int(seed_off[j]):int(seed_off[j + 1])] for j in range(2 * N)]
    lens = [len(q) for q in R.reads[:N]]
    off2 = scan([x for m in lens for x in (m, m)])
    coins = np.random.default_rng(5).integers(0, 2, N).astype(np.uint8)
    c2 = Case(R, 1)
    d_seeds = c2.inp("d_seeds", np.array(sel_recs, np.uint64).reshape(-1), 8)
    d_soff, d_off2, d_coins = c2.inp("d_seed_off", np.array(seed_off, np.uint64)), c2.inp("d_off2", off2), c2.inp("d_first_fwd", coins, 1)
    stmp_bytes = int(L.rbg_report_select_tmp_bytes(N))
    stmp = c2.out("d_select_tmp", stmp_bytes, 8)
    c2.freeze()
    sel = []
    for tag, kw, use_coins, with_read in (("default", dict(), False, True), ("heuristic", dict(heuristic=True, best_strand=True, min_seed_len=20, read_len=REPORT_READ_LEN), True, False),
                                          ("heuristic_nocoin", dict(heuristic=True, min_seed_len=12, read_len=REPORT_READ_LEN), False, True)):
        params = capi.report_params(**kw)
        rep_off, d_out = c2.u64(f"d_rep_off_{tag}", N + 1), c2.out(f"d_out_{tag}", 48 * S_reads, 8)
        d_read = c2.out(f"d_out_read_{tag}", 4 * S_reads, 4) if with_read else None
        import ctypes
        args = (rb.h, d_seeds.ptr, d_soff.ptr, d_off2.ptr, N, d_coins.ptr if use_coins else None, ctypes.byref(params), rep_off.ptr, d_out.ptr,
                d_read.ptr if d_read else None, stmp.ptr)
        if tag == "default":
            refused(c2, *[(L.rbg_report_select_dev, *args, declared, st) for declared in (stmp_bytes - 1, 0)])
        assert L.rbg_report_select_dev(*args, stmp_bytes, st) == 0
        want = _select_model(sel_by_seq, lens, coins if use_coins else None, bool(kw.get("heuristic")), bool(kw.get("best_strand")), kw.get("min_seed_len", 0),
                             REPORT_READ_LEN)
        sel.append((rep_off, d_out, d_read, want))
    c2.sync_and_check()
    for rep_off, d_out, d_read, want in sel:
        _check_selected(c2, rep_off, d_out, d_read, want, S_reads)
    if N >= 63:
        assert len(sel[0][3][1]) > len(sel[1][3][1]) > 0


MANY_READS = 24000


@pytest.fixture(scope="module")
def many_ref(ref):
    """24000 synthetic reads with up to two records per strand and up to three markers per record (sorted and unique, as the canon leaves them); one
    record in twenty has an empty range"""
    rng = np.random.default_rng(41)
    N = MANY_READS
    lens = rng.integers(30, 121, N).tolist()
    pool = [int(v) for v in ref.markers[3][:60]]
    by_seq, recs, mk, seed_off = [], [], [], [0]
    for j in range(2 * N):
        w = []
        m_len = lens[j // 2]
        for _ in range(int(rng.integers(0, 3))):
            m = sorted({pool[int(t)] for t in rng.integers(0, len(pool), int(rng.integers(0, 4)))}, key=RM.marker_key)
            qs, lo, d = int(rng.integers(0, m_len)), int(rng.integers(2, 1000)), int(rng.integers(0, 100))
            rec = [lo, lo + d % 5 - (2 if d < 5 else 0), qs, qs + d % (m_len - qs + 1), len(mk), len(mk) + len(m)]
            mk += m
            w.append(rec)
        by_seq.append(w)
        recs += w
        seed_off.append(len(recs))
    want = _select_model(by_seq, lens, None, False, False, 0, REPORT_READ_LEN)
    table = {}
    for range_size, qstart, qlen, b, e, strand in want[1]:
        for m in mk[b:e]:
            t = table.setdefault(m, [0, 0, 0])
            t[strand] += 1
            t[2] = (t[2] + qlen) & M64
    return lens, recs, mk, seed_off, want, table, len(pool)


@forms
def test_report_select_and_tally_with_scans_of_many_blocks(ref, many_ref, handles, form):
    """24000 synthetic reads (no index behind them: select sees records and lengths only), so that the scans of rbg_report_select_dev (over the reads) and of
    rbg_tally_add_dev / rbg_tally_add_reads_dev (over some 45000 printed records) take many blocks, each on a scratch of exact size at 8-byte alignment,
    skew 8 -- a scan's block states are 16-byte units.  Select against the model above; the tallies (line mode) against a count in Python: per marker the
    lines that carry it by strand, and the sum of their query lengths."""
    import ctypes
    rb, R = handles(form), ref
    N = MANY_READS
    lens, recs, mk, seed_off, want, table, npool = many_ref
    S = len(recs)
    c = Case(R, 1, arena_bytes=32 << 20)
    L, st = c.L, c.st
    d_seeds = c.inp("d_seeds", np.array(recs, np.uint64).reshape(-1), 8)
    d_soff, d_off2 = c.inp("d_seed_off", np.array(seed_off, np.uint64)), c.inp("d_off2", scan([x for m in lens for x in (m, m)]))
    d_mk = c.inp("d_mk", np.array(mk, np.uint64))
    stmp_bytes = int(L.rbg_report_select_tmp_bytes(N))
    stmp = c.out("d_select_tmp", stmp_bytes, 8)
    rep_off, d_out, d_read = c.u64("d_rep_off", N + 1), c.out("d_out", 48 * S, 8), c.out("d_out_read", 4 * S, 4)
    params = capi.report_params()
    c.freeze()
    assert L.rbg_report_select_dev(rb.h, d_seeds.ptr, d_soff.ptr, d_off2.ptr, N, None, ctypes.byref(params), rep_off.ptr, d_out.ptr, d_read.ptr, stmp.ptr,
                                   stmp_bytes, st) == 0
    c.sync_and_check()
    _check_selected(c, rep_off, d_out, d_read, want, S)
    Rn = len(want[1])
    assert 40000 < Rn < S
    M_upper = sum(r[4] - r[3] for r in want[1])
    c.freeze("d_out", "d_rep_off")
    b1, b2 = int(L.rbg_tally_add_tmp_bytes(Rn)), int(L.rbg_tally_add_reads_tmp_bytes(N, Rn))
    tmp1, tmp2 = c.out("d_tally_tmp", b1, 8), c.out("d_tally_reads_tmp", b2, 8)
    t1, t2 = capi.Tally(rb, npool), capi.Tally(rb, npool)
    try:
        t1.reserve(M_upper)
        t2.reserve(M_upper)
        assert L.rbg_tally_add_dev(t1.h, d_out.ptr, Rn, d_mk.ptr, M_upper, tmp1.ptr, b1, st) == 0
        assert L.rbg_tally_add_reads_dev(t2.h, d_out.ptr, Rn, rep_off.ptr, N, d_mk.ptr, M_upper, 0, tmp2.ptr, b2, st) == 0
        c.sync_and_check()
        for t in (t1, t2):
            got = {int(e["marker"]): [int(e["n_fwd"]), int(e["n_rev"]), int(e["len_sum"])] for e in t.export()}
            assert got == table
    finally:
        t1.close()
        t2.close()


# ---- the walks ------------------------------------------------------------------------------------------------------------------------------------------
import fl_model as FM          # noqa: E402
import sam_extend_model as XM  # noqa: E402

WALK_M = 500
WALK_K = 4
ZERO_WALK = dict(ext=0, nm=0, score=0, steps=0, mis=[], why="skip")


@pytest.fixture(scope="module")
def walk_ref(ref):
    """500 items over rows of the synth index, each with a sequence of its own: `a` bases left of the occurrence (with substitutions, an N, a lower-case
    base), the `skip` bases of the seed as the text has them, a right flank with substitutions.  The left walk starts at a, the right walk at b = a + skip;
    the references are sam_extend_model.walk_bases and fl_model.walk_right over the TEXT, FL is the text's next suffix."""
    S = ref.S
    n, text, sa = S.n, S.text, S.fm.sa
    isa = np.empty(n, np.int64)
    isa[sa] = np.arange(n)
    rng = np.random.default_rng(12)
    rows = rng.choice(n, WALK_M, replace=False)
    rows[:3] = [int(isa[n - 1]), int(isa[0]), int(isa[n - 2])]              # the terminator's row, the row of text position 0, the last base
    seqs, W = [], dict(a=[], b=[], row=[], skip=[], llim=[], rlim=[], left=[], right=[], sym=[], nxt=[])

    def mutate(buf, where, j):
        for p in where:
            buf[p] = ord("ACGT"[("ACGT".index(chr(buf[p])) + 1 + j % 3) % 4]) if chr(buf[p]) in "ACGT" else ord("C")

    for j, r in enumerate(int(x) for x in rows):
        l = int(sa[r])
        a, skip, tail = (j * 7) % 71, (j * 5) % 31, 10 + (j * 11) % 61
        pre = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), max(a - l, 0)).tobytes() + text[max(l - a, 0):l].tobytes())
        mutate(pre, rng.choice(a, min(j % 7, a), replace=False) if a else [], j)
        if j % 13 == 5 and a > 3:
            pre[a - 3] = ord("N")
        body = bytearray(text[l:l + skip + tail].tobytes())
        body += bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), skip + tail - len(body)).tobytes())
        mutate(body, [skip + int(p) for p in rng.choice(tail, min(j % 7, tail), replace=False)], j)
        if j % 17 == 3:
            body[skip + 6] = ord(chr(body[skip + 6]).lower())
        s = bytes(pre) + bytes(body)
        seqs.append(s)
        llim, rlim = (0, 1, a, a + 5, 1 << 40)[j % 5], (1 << 40, 0, 1, tail, tail + 5)[j % 5]
        W["a"].append(a); W["b"].append(a + skip); W["row"].append(r); W["skip"].append(skip); W["llim"].append(llim); W["rlim"].append(rlim)
        W["left"].append(XM.walk_bases(s, a, min(a, llim), WALK_K, lambda t: int(text[(l - 1 - t) % n])))
        if any(int(text[(l + x) % n]) not in b"ACGT" for x in range(skip)):
            W["right"].append(ZERO_WALK)
        else:
            W["right"].append(FM.walk_right(s, a + skip, min(len(s) - a - skip, rlim), WALK_K, lambda t: int(text[(l + skip + t) % n])))
        base = int(text[l]) in b"ACGT"
        W["sym"].append(int(text[l]) if base else 0)
        W["nxt"].append(int(isa[l + 1]) if base else MAXU)
    perm = rng.permutation(WALK_M)                                          # item j reads sequence perm[j]
    packed, off = ra.pack_reads([seqs[j] for j in np.argsort(perm)])
    assert {x["why"] for x in W["left"]} == {"length", "budget", "base"} and {"length", "budget"} <= {x["why"] for x in W["right"]}
    assert any(x["nm"] for x in W["left"][:63]) and any(x["nm"] for x in W["right"][:63]) and 0 in W["sym"][:3]
    return packed, off, perm.astype(np.uint32), W


def _walk_records(region, M):
    g = region.numpy().view(capi.EXTEND)
    assert len(g) == M
    return [(int(x["ext"]), int(x["nm"]), int(x["score"]), int(x["steps"]), tuple(int(v) for v in x["mis_t"]), tuple(int(v) for v in x["mis_ref"])) for x in g]


@forms
@pytest.mark.parametrize("M", [1, 63, 65, WALK_M])
def test_walks(ref, walk_ref, handles, form, M):
    """rbg_extend_left_dev, rbg_fl_dev and rbg_extend_right_dev over the first M items: d_out holds 56-byte records at 4-byte alignment, exactly M of them.
    Then the same calls with an item error in the middle (an a / b beyond its sequence, a row >= n): the call answers RBG_EARG after running, that item's
    record is zero (sym 0, next 0), the neighbours' records are right, guards and inputs untouched."""
    rb, R = handles(form), ref
    packed, off, perm, W = walk_ref
    assert capi.EXTEND.itemsize == 56
    Nw = len(off) - 1
    c = Case(R, 1)
    L, st = c.L, c.st
    body = np.zeros(up16(len(packed)), np.uint8)
    body[:len(packed)] = packed
    seqs, d_off = c.inp("d_wseqs", body, 16), c.inp("d_woff", off)
    mid = M // 2
    col = lambda key, dt: np.array(W[key][:M], dt)
    bad = lambda arr, v: np.where(np.arange(M) == mid, v, arr).astype(arr.dtype)
    a, b, row, skip, llim, rlim = col("a", np.uint32), col("b", np.uint32), col("row", np.uint64), col("skip", np.uint32), col("llim", np.uint64), col("rlim", np.uint64)
    d_seq = c.inp("d_item_seq", perm[:M], 4)
    d_a, d_b, d_skip = c.inp("d_item_a", a, 4), c.inp("d_item_b", b, 4), c.inp("d_item_skip", skip, 4)
    d_row, d_llim, d_rlim = c.inp("d_item_row", row), c.inp("d_item_llim", llim), c.inp("d_item_rlim", rlim)
    d_a_bad, d_b_bad, d_row_bad = c.inp("d_item_a_bad", bad(a, 5000), 4), c.inp("d_item_b_bad", bad(b, 5000), 4), c.inp("d_item_row_bad", bad(row, R.S.n))
    outs = {k: c.out("d_out_" + k, 56 * M, 4) for k in ("left", "right", "left_bad", "right_bad")}
    sym, nxt = c.out("d_sym", M, 1), c.u64("d_next", M)
    sym_bad, nxt_bad = c.out("d_sym_bad", M, 1), c.u64("d_next_bad", M)
    c.freeze()
    assert L.rbg_extend_left_dev(rb.h, seqs.ptr, d_off.ptr, Nw, d_seq.ptr, d_a.ptr, d_row.ptr, d_llim.ptr, M, WALK_K, outs["left"].ptr, st) == 0
    assert L.rbg_extend_right_dev(rb.h, seqs.ptr, d_off.ptr, Nw, d_seq.ptr, d_b.ptr, d_row.ptr, d_skip.ptr, d_rlim.ptr, M, WALK_K, outs["right"].ptr, st) == 0
    assert L.rbg_fl_dev(rb.h, d_row.ptr, M, sym.ptr, nxt.ptr, st) == 0
    c.sync_and_check()
    want_l, want_r = [XM.record_tuple(x) for x in W["left"][:M]], [XM.record_tuple(x) for x in W["right"][:M]]
    assert _walk_records(outs["left"], M) == want_l
    assert _walk_records(outs["right"], M) == want_r
    same(sym, W["sym"][:M], np.uint8)
    same(nxt, W["nxt"][:M])
    # the item errors: reported when the kernel has run
    assert L.rbg_extend_left_dev(rb.h, seqs.ptr, d_off.ptr, Nw, d_seq.ptr, d_a_bad.ptr, d_row.ptr, d_llim.ptr, M, WALK_K, outs["left_bad"].ptr, st) == EARG
    assert L.rbg_extend_right_dev(rb.h, seqs.ptr, d_off.ptr, Nw, d_seq.ptr, d_b_bad.ptr, d_row.ptr, d_skip.ptr, d_rlim.ptr, M, WALK_K, outs["right_bad"].ptr, st) == EARG
    assert L.rbg_fl_dev(rb.h, d_row_bad.ptr, M, sym_bad.ptr, nxt_bad.ptr, st) == EARG
    c.sync_and_check()
    zero = XM.record_tuple(ZERO_WALK)
    assert _walk_records(outs["left_bad"], M) == want_l[:mid] + [zero] + want_l[mid + 1:]
    assert _walk_records(outs["right_bad"], M) == want_r[:mid] + [zero] + want_r[mid + 1:]
    same(sym_bad, W["sym"][:mid] + [0] + W["sym"][mid + 1:M], np.uint8)
    same(nxt_bad, W["nxt"][:mid] + [0] + W["nxt"][mid + 1:M])
    # a budget above RBG_SAM_MAX_MISMATCH is refused before anything runs
    refused(c, (L.rbg_extend_left_dev, rb.h, seqs.ptr, d_off.ptr, Nw, d_seq.ptr, d_a.ptr, d_row.ptr, d_llim.ptr, M, 9, outs["left"].ptr, st),
            (L.rbg_extend_right_dev, rb.h, seqs.ptr, d_off.ptr, Nw, d_seq.ptr, d_b.ptr, d_row.ptr, d_skip.ptr, d_rlim.ptr, M, 9, outs["right"].ptr, st))
