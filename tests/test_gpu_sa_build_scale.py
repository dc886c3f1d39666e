"""rbg_suffix_array_dev and rbg_text_runs_plan_dev / _fill_dev (rowbowt_amd/csrc/sa_build.hip) where tests/test_gpu_sa_build.py does not go: past one pass
of the grid-stride loop, through every sort variant at both position widths, on a stream that is busy, on scratch that is not fresh, at every refusal,
and through the host path at 8-byte positions.  The inputs and the counter model are tests/sa_scale_cases.py (checked without a device in
tests/test_sa_scale_expected.py); the helpers and the guarded arena are those of tests/test_gpu_sa_build.py.

The grid is capped at CAP = 8 192 x 256 lanes, so a lane handles a second element only where a kernel runs over more than CAP elements: the boundary
texts put n on either side of CAP (and of rocPRIM's merge-sort limit 2^20); the near-copies text keeps 2 998 749 of its 3 000 030 suffixes listed after
the first key, so rounds 1 to 11 stride the grid as well and the list crosses the merge-sort limit on the way down (round 15 sorts 1 196 316 suffixes,
round 16 sorts 277 980), 17 rounds in all; the long run sorts nearly all n = CAP + 301 suffixes in every one of 20 rounds.  The reference is the torch prefix doubling of rowbowt_amd/tools/synth_pangenome.py on the device (the long
run: its closed form), made once per text and shared by both widths.  rounds, sorted and tied_after_first are asserted EXACTLY against
sa_scale_cases.counter_model, which derives them from the LCP array -- a compaction that kept a suffix too many would pass every comparison of arrays."""
import functools

import numpy as np
import pytest
import torch

import naive
import rowbowt_amd as ra
import sa_scale_cases as SC
from arena import Arena
from rowbowt_amd import capi
from rowbowt_amd.tools import synth_pangenome as SP
from sa_scale_cases import CAP, MERGE_LIMIT
from test_gpu_sa_build import EARG, check_info, run_runs, run_sa

pytestmark = pytest.mark.gpu
COUNTERS = ("rounds", "sorted", "tied_after_first")
RUN_ARRAYS = ("heads", "lens", "ssa", "esa")
MID = f"boundary n={MERGE_LIMIT + 1}"


@functools.lru_cache(maxsize=None)
def scale_expected(name):
    """(text, suffix array, (heads, lens, ssa, esa), counters) on the host: made once per text, shared by the widths and the tests"""
    t = SC.scale_texts()[name]()
    if name == "long run":
        sa = SC.long_run_sa(len(t))
        runs = SC.runs_from_sa(t, sa)
    else:
        d_text = torch.from_numpy(t).cuda()
        d_sa = SP.suffix_array(d_text)
        ref = SP.index_inputs(d_text, d_sa)
        sa, runs = d_sa.cpu().numpy(), tuple(ref[k] for k in RUN_ARRAYS)
    return t, sa, runs, SC.counter_model(t, sa)


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    scale_expected.cache_clear()


def assert_rows(name, pb, got, sa):
    bad = np.flatnonzero(got.astype(np.int64) != sa)
    assert len(bad) == 0, "%s at %d-byte positions: %d rows differ, the first at %s (grid pass %s): got %s, expected %s" % (
        name, pb, len(bad), bad[:5], bad[:5] // CAP, got[bad[:5]], sa[bad[:5]])


def assert_runs(name, pb, got, want, upto=None):
    """the run arrays; a difference is reported with the run's first row and the grid pass that row falls in"""
    first_row = np.cumsum(want[1].astype(np.int64)) - want[1].astype(np.int64)
    for what, a, b in zip(RUN_ARRAYS, got, want):
        a, b = a[:upto], b[:upto]
        assert a.shape == b.shape, (name, pb, what, a.shape, b.shape)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, "%s at %d-byte positions: %s differs at %d runs, the first %s (first rows %s, grid pass %s): got %s, expected %s" % (
            name, pb, what, len(bad), bad[:5], first_row[bad[:5]], first_row[bad[:5]] // CAP, a[bad[:5]], b[bad[:5]])


def assert_counters(name, pb, model):
    info = capi.sa_info()
    assert {k: info[k] for k in COUNTERS} == model, (name, pb, info, model)


# ---- 1. the suffix array, the runs and the counters at scale ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pb", [4, 8])
@pytest.mark.parametrize("name", list(SC.scale_texts()))
def test_suffix_array_runs_and_counters_at_scale(name, pb):
    t, sa, runs, model = scale_expected(name)
    got, A, d_text, d_sa = run_sa(t, pb)
    assert_rows(name, pb, got, sa)
    check_info(len(t), pb)
    assert_counters(name, pb, model)
    assert_runs(name, pb, run_runs(A, d_text, d_sa, len(t), pb, len(runs[0])), runs)


# ---- 2. a side stream that is actually used ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pb", [4, 8])
def test_a_side_stream_that_is_busy(pb):
    """The text region of the arena holds the pattern byte until a copy on the side stream fills it, and that copy is queued behind matrix products that
    are still running when rbg_suffix_array_dev is called with the stream's handle; nothing is synchronised until the fill has been queued, and then that
    stream only.  A kernel, memset, copy or hipCUB call that went to the null stream or to another stream would read the text (or what the step before
    it wrote) too early and break the terminator rule or the comparison.  When the code is right the test passes deterministically; a mis-streamed launch
    is detected only with high probability (it has about 40 ms of queued work to overtake), not with certainty.  The same is done again before the
    plan and before the fill, with the suffix array put aside and the pattern in its place until the queued work is through."""
    t, sa, runs, model = scale_expected(MID)
    L = ra.lib()
    n, R = len(t), len(runs[0])
    nb, nbr = int(L.rbg_sa_tmp_bytes(n, pb)), int(L.rbg_text_runs_tmp_bytes(n, pb))
    A = Arena(n + n * pb + nb + nbr + 25 * R + 16384, device="cuda")
    d_text = A.carve("text", n, align=1)
    d_sa = A.carve("sa", n * pb, align=pb)
    d_tmp = A.carve("tmp", nb, align=256)
    d_rtmp = A.carve("runs tmp", nbr, align=256)
    heads = A.carve("heads", R, align=1)
    lens, ssa, esa = (A.carve(k, R * 8, align=8) for k in RUN_ARRAYS[1:])
    staging = torch.from_numpy(t).cuda()
    x = torch.randn(8192, 8192, device="cuda")
    y = x @ x                                          # (the library's first call, outside the part that must stay asynchronous)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    st = side.cuda_stream
    Rg = capi.U64()

    def behind_work(then):
        """on the side stream: matrix products, then `then`; the stream is still busy when this returns"""
        with torch.cuda.stream(side):
            for _ in range(6):
                torch.matmul(x, x, out=y)
            then()
        assert not side.query(), "the side stream has run dry before the call: the test would prove nothing"

    try:
        behind_work(lambda: d_text.u8.copy_(staging, non_blocking=True))
        rc = L.rbg_suffix_array_dev(d_text.ptr, n, d_sa.ptr, pb, d_tmp.ptr, nb, st)
        # the call has waited for the stream, so its result is put aside and comes back only behind more work: the plan and the fill find the pattern
        # in d_sa (a value that is no text position, which bwt_at reads as position 0: nothing out of bounds) unless they run where they were told to
        with torch.cuda.stream(side):
            kept = d_sa.u8.clone()
            d_sa.fill(A.pattern)
        behind_work(lambda: d_sa.u8.copy_(kept))
        rc_plan = L.rbg_text_runs_plan_dev(d_text.ptr, d_sa.ptr, n, pb, d_rtmp.ptr, nbr, capi.C.byref(Rg), st)
        with torch.cuda.stream(side):
            d_sa.fill(A.pattern)
        behind_work(lambda: (d_sa.u8.copy_(kept), lens.fill(0x5A)))      # (lens: the fill zeroes it first, on its stream)
        rc_fill = L.rbg_text_runs_fill_dev(d_text.ptr, d_sa.ptr, n, pb, d_rtmp.ptr, nbr, R, heads.ptr, lens.ptr, ssa.ptr, esa.ptr, st)
    finally:
        side.synchronize()                             # (that stream only; also before a failure lets go of the arena)
    assert (rc, rc_plan, rc_fill) == (0, 0, 0) and int(Rg.value) == R, (rc, rc_plan, rc_fill, int(Rg.value), R)
    A.check()
    assert (d_text.numpy() == t).all()
    assert_rows(MID, pb, d_sa.numpy(np.uint32 if pb == 4 else np.uint64), sa)
    assert_counters(MID, pb, model)
    assert_runs(MID, pb, (heads.numpy(), lens.numpy(np.uint64), ssa.numpy(np.uint64), esa.numpy(np.uint64)), runs)


# ---- 3. scratch and outputs that are not fresh ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pb", [4, 8])
def test_scratch_and_outputs_that_are_not_fresh(pb):
    """a large text, then A*257 in the same d_sa, d_tmp, runs scratch and run arrays, none of them refilled: the small result is exact and everything
    behind it is still the large one"""
    t, sa, runs, _ = scale_expected(MID)
    small = SC.long_run(257)
    small_sa = SC.long_run_sa(len(small))
    small_runs = SC.runs_from_sa(small, small_sa)
    L = ra.lib()
    st = torch.cuda.current_stream().cuda_stream
    n, ns, R, Rs = len(t), len(small), len(runs[0]), len(small_runs[0])
    dt = np.uint32 if pb == 4 else np.uint64
    nb, nbr = int(L.rbg_sa_tmp_bytes(n, pb)), int(L.rbg_text_runs_tmp_bytes(n, pb))
    A = Arena(n + ns + n * pb + nb + nbr + 25 * R + 16384, device="cuda")
    d_text = A.carve_from("text", t, align=1)
    d_small = A.carve_from("small text", small, align=1)
    d_sa = A.carve("sa", n * pb, align=pb)
    d_tmp = A.carve("tmp", nb, align=256)
    d_rtmp = A.carve("runs tmp", nbr, align=256)
    heads = A.carve("heads", R, align=1)
    lens, ssa, esa = (A.carve(k, R * 8, align=8) for k in RUN_ARRAYS[1:])
    A.snapshot_all(["text", "small text"])
    Rg = capi.U64()

    def build(d, m, r):
        assert L.rbg_suffix_array_dev(d.ptr, m, d_sa.ptr, pb, d_tmp.ptr, nb, st) == 0
        assert L.rbg_text_runs_plan_dev(d.ptr, d_sa.ptr, m, pb, d_rtmp.ptr, nbr, capi.C.byref(Rg), st) == 0 and int(Rg.value) == r, (int(Rg.value), r)
        assert L.rbg_text_runs_fill_dev(d.ptr, d_sa.ptr, m, pb, d_rtmp.ptr, nbr, r, heads.ptr, lens.ptr, ssa.ptr, esa.ptr, st) == 0
        torch.cuda.synchronize()
        A.check(), A.assert_all_unchanged()
        return d_sa.numpy(dt), (heads.numpy(), lens.numpy(np.uint64), ssa.numpy(np.uint64), esa.numpy(np.uint64))

    got, got_runs = build(d_text, n, R)
    assert_rows(MID, pb, got, sa)
    assert_runs(MID, pb, got_runs, runs)
    before = {k: A[k].numpy() for k in ("sa",) + RUN_ARRAYS}
    got, got_runs = build(d_small, ns, Rs)
    assert_rows("A*257 after " + MID, pb, got[:ns], small_sa)
    assert_counters("A*257 after " + MID, pb, SC.counter_model(small, small_sa))
    assert_runs("A*257 after " + MID, pb, got_runs, small_runs, upto=Rs)
    A.check_untouched("sa", [(ns * pb, n * pb)], expect=before["sa"])
    A.check_untouched("heads", [(Rs, R)], expect=before["heads"])
    for k in RUN_ARRAYS[1:]:
        A.check_untouched(k, [(Rs * 8, R * 8)], expect=before[k])


# ---- 4. refusals leave the outputs untouched ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pb", [4, 8])
def test_refusals_leave_the_outputs_untouched(pb):
    """every argument the header refuses, one at a time beside arguments that are otherwise those of a call that succeeds (the calls at the end do):
    RBG_EARG, and d_sa, both scratch areas, *R and the run arrays as they were"""
    t = SC.boundary_text(1025)
    n = len(t)
    sa = np.asarray(naive.suffix_array(t), np.int64)
    runs = SC.runs_from_sa(t, sa)
    R = len(runs[0])
    L = ra.lib()
    st = torch.cuda.current_stream().cuda_stream
    nb, nbr = int(L.rbg_sa_tmp_bytes(n, pb)), int(L.rbg_text_runs_tmp_bytes(n, pb))
    assert nb and nbr and L.rbg_sa_tmp_bytes(n, 0) == L.rbg_sa_tmp_bytes(n, 2) == L.rbg_sa_tmp_bytes(n, 16) == 0
    assert L.rbg_text_runs_tmp_bytes(n, 0) == L.rbg_text_runs_tmp_bytes(n, 2) == L.rbg_text_runs_tmp_bytes(n, 16) == 0
    A = Arena(n + (n + 1) * pb + nb + nbr + 25 * R + 16384, device="cuda")
    d_text = A.carve_from("text", t, align=1)
    d_sa = A.carve("sa", (n + 1) * pb, align=pb)       # (an entry to spare: the misaligned d_sa still has n entries of room)
    d_tmp = A.carve("tmp", nb + 256, align=256)        # (the same for a d_tmp off its alignment)
    d_rtmp = A.carve("runs tmp", nbr + 256, align=256)
    heads = A.carve("heads", R, align=1)
    lens, ssa, esa = (A.carve(k, R * 8, align=8) for k in RUN_ARRAYS[1:])
    A.snapshot("text")
    Rg = capi.U64(12345)
    outputs = ["sa", "tmp", "runs tmp"] + list(RUN_ARRAYS)
    state = {}

    def keep():
        state.update({k: A[k].numpy() for k in outputs})

    def refused(what, rc, r_was=12345):
        torch.cuda.synchronize()
        assert rc == EARG, (what, rc)
        assert int(Rg.value) == r_was, (what, int(Rg.value))
        A.check(), A.assert_all_unchanged()
        for k in outputs:
            A.check_untouched(k, [(0, A[k].nbytes)], expect=state[k])

    def sa_call(**kw):
        a = dict(text=d_text.ptr, n=n, sa=d_sa.ptr, pb=pb, tmp=d_tmp.ptr, nb=nb)
        a.update(kw)
        return L.rbg_suffix_array_dev(a["text"], a["n"], a["sa"], a["pb"], a["tmp"], a["nb"], st)

    def plan_call(**kw):
        a = dict(text=d_text.ptr, sa=d_sa.ptr, n=n, pb=pb, tmp=d_rtmp.ptr, nb=nbr, R=capi.C.byref(Rg))
        a.update(kw)
        return L.rbg_text_runs_plan_dev(a["text"], a["sa"], a["n"], a["pb"], a["tmp"], a["nb"], a["R"], st)

    def fill_call(**kw):
        a = dict(text=d_text.ptr, sa=d_sa.ptr, n=n, pb=pb, tmp=d_rtmp.ptr, nb=nbr, R=R, heads=heads.ptr, lens=lens.ptr, ssa=ssa.ptr, esa=esa.ptr)
        a.update(kw)
        return L.rbg_text_runs_fill_dev(a["text"], a["sa"], a["n"], a["pb"], a["tmp"], a["nb"], a["R"], a["heads"], a["lens"], a["ssa"], a["esa"], st)

    widths = [dict(pb=0), dict(pb=2), dict(pb=16)]
    off_sa = [dict(sa=d_sa.ptr + 1), dict(sa=d_sa.ptr + pb // 2)]
    keep()
    for c in [dict(nb=nb - 1), dict(tmp=d_tmp.ptr + 8), dict(tmp=d_tmp.ptr + 128), dict(text=None), dict(sa=None), dict(tmp=None), dict(n=0)] + off_sa + widths:
        refused(("rbg_suffix_array_dev", c), sa_call(**c))
    assert sa_call() == 0
    torch.cuda.synchronize()
    assert_rows("refusals", pb, d_sa.numpy(np.uint32 if pb == 4 else np.uint64)[:n], sa)
    keep()
    for c in [dict(nb=nbr - 1), dict(tmp=d_rtmp.ptr + 8), dict(tmp=d_rtmp.ptr + 128), dict(text=None), dict(sa=None), dict(tmp=None), dict(R=None),
              dict(n=0)] + off_sa + widths:
        refused(("rbg_text_runs_plan_dev", c), plan_call(**c))
    assert plan_call() == 0 and int(Rg.value) == R
    torch.cuda.synchronize()
    keep()
    for c in [dict(nb=nbr - 1), dict(tmp=d_rtmp.ptr + 8), dict(tmp=d_rtmp.ptr + 128), dict(text=None), dict(sa=None), dict(tmp=None), dict(heads=None),
              dict(lens=None), dict(ssa=None), dict(esa=None), dict(n=0), dict(R=0), dict(R=n + 1)] + off_sa + widths:
        refused(("rbg_text_runs_fill_dev", c), fill_call(**c), r_was=R)
    assert fill_call() == 0
    torch.cuda.synchronize()
    A.check(), A.assert_all_unchanged()
    assert_runs("refusals", pb, (heads.numpy(), lens.numpy(np.uint64), ssa.numpy(np.uint64), esa.numpy(np.uint64)), runs)


# ---- 5. a run count that is not the plan's -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pb", [4, 8])
def test_fill_with_one_run_fewer_than_the_plan_counted(pb):
    """include/rbg.h: with a smaller R the call returns 0, writes the first R runs in full and nothing behind entry R - 1 -- arrays of R - 1 entries on
    the arena, on a small text and on one whose last run lies in the second grid pass"""
    for name, t, sa, runs in (("boundary n=1025", SC.boundary_text(1025), None, None), (f"boundary n={CAP + 1}",) + scale_expected(f"boundary n={CAP + 1}")[:3]):
        if sa is None:
            sa = np.asarray(naive.suffix_array(t), np.int64)
            runs = SC.runs_from_sa(t, sa)
        n, R = len(t), len(runs[0])
        assert R >= 8
        L = ra.lib()
        st = torch.cuda.current_stream().cuda_stream
        got, A, d_text, d_sa = run_sa(t, pb)
        assert_rows(name, pb, got, sa)
        nbr = int(L.rbg_text_runs_tmp_bytes(n, pb))
        B = Arena(nbr + 25 * R + 8192, device="cuda")
        d_rtmp = B.carve("runs tmp", nbr, align=256)
        Rg = capi.U64()
        assert L.rbg_text_runs_plan_dev(d_text.ptr, d_sa.ptr, n, pb, d_rtmp.ptr, nbr, capi.C.byref(Rg), st) == 0 and int(Rg.value) == R
        heads = B.carve("heads", R - 1, align=1)
        lens, ssa, esa = (B.carve(k, (R - 1) * 8, align=8) for k in RUN_ARRAYS[1:])
        A.snapshot("sa")
        assert L.rbg_text_runs_fill_dev(d_text.ptr, d_sa.ptr, n, pb, d_rtmp.ptr, nbr, R - 1, heads.ptr, lens.ptr, ssa.ptr, esa.ptr, st) == 0
        torch.cuda.synchronize()
        A.check(), B.check(), A.assert_all_unchanged()
        assert_runs(name, pb, (heads.numpy(), lens.numpy(np.uint64), ssa.numpy(np.uint64), esa.numpy(np.uint64)), runs, upto=R - 1)


# ---- 6. the host path at 8-byte positions --------------------------------------------------------------------------------------------------------
def _host_text(name):
    import extract_wide_cases as EW
    import isa_model as IM
    return IM.synth_text() if name == "synth" else EW.docs()


@pytest.mark.parametrize("name", ["synth", "docs"])
def test_from_text_at_8_byte_positions(name):
    import sweeps
    from test_gpu_build_text import ARRAYS
    T = _host_text(name)
    with capi.default_option(capi.OPT_POS_BYTES, 8), capi.default_option(capi.OPT_RANK_LAYOUT, capi.LAYOUT_RUNS):
        rb = ra.RowBowt.from_text(T.tb, device=0)
        built = capi.sa_info()
        want = ra.RowBowt.from_runs(T.heads, T.lens, T.ssa, T.esa, device=0)
        try:
            assert built["pos_bytes"] == 8 and built["n"] == T.n, built
            assert {k: built[k] for k in COUNTERS} == SC.counter_model(T.text, T.sa), built
            assert rb.info().pos_bytes == 8 and want.info().pos_bytes == 8 and rb.info().n == T.n and rb.info().r == len(T.heads) and rb.info().has_tsa == 1
            for which in ARRAYS:
                assert (rb.host_array(which) == want.host_array(which)).all(), which
            sweeps.run_sweep_c("%s from_text at 8-byte positions" % name, rb, sweeps.sweep_c(sweeps.Index(T.text, T.sa).ref))
        finally:
            rb.close(), want.close()


def test_convert_text_at_8_byte_positions(tmp_path):
    T = _host_text("docs")
    docs_text = "".join(f"{n} {s}\n" for n, s in zip(T.doc_names, T.doc_starts))
    a, b = tmp_path / "text.rbgpu", tmp_path / "runs.rbgpu"
    with capi.default_option(capi.OPT_POS_BYTES, 8):
        capi.convert_text(T.tb, a, docs_text=docs_text)
        assert capi.sa_info()["pos_bytes"] == 8 and capi.sa_info()["n"] == T.n
        capi.convert_runs(T.heads, T.lens, T.ssa, T.esa, out_path=b, docs_text=docs_text)
    assert a.read_bytes() == b.read_bytes()
