"""GPU parity of rbg_fl_dev (fl_extend.hip k_fl_rows over the FL index of rbg_fl_prepare) against the text itself: at every row of a 2 051-symbol pangenome
sym = text[SA[row]] and FL = ISA[SA[row] + 1] (text_ref.TextRef; no oracle), on both layouts at 4-byte and forced 8-byte positions; and on a run list whose
lengths carry rows across 2^32 against tests/fl_model.py."""
import numpy as np
import pytest

import fl_model as FM
import rowbowt_amd as ra
from rowbowt_amd import capi
from gpu_common import _random_run_index, _with_layout
from synth import SynthIndex
from text_ref import TextRef

pytestmark = pytest.mark.gpu
EARG, ENOTLOADED = -4, -6
MAXU = 2**64 - 1


@pytest.fixture(scope="module")
def small():
    S = SynthIndex(L=400, H=5, n_sites=12, seed=41)
    T = TextRef(S.text, S.fm.sa)
    n = S.n
    base = np.isin(T.text[T.sa], np.frombuffer(b"ACGT", np.uint8))
    sym = np.where(base, T.text[T.sa], 0).astype(np.uint8)
    nxt = np.where(base, T.isa[(T.sa + 1) % n], -1).astype(np.int64).view(np.uint64)
    assert n == 2051 and int((~base).sum()) == 1
    return S, T, sym, nxt


@pytest.fixture(scope="module", params=[(capi.LAYOUT_SLOTS, 0), (capi.LAYOUT_RUNS, 0), (capi.LAYOUT_SLOTS, 8), (capi.LAYOUT_RUNS, 8)],
                ids=["slots", "runs", "slots-8-byte", "runs-8-byte"])
def rb(request, small):
    S = small[0]
    layout, pos_bytes = request.param
    with capi.default_option(capi.OPT_POS_BYTES, pos_bytes):
        h = _with_layout(layout, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    assert h.info().pos_bytes == (pos_bytes or 4)
    yield h
    h.close()


def _not_loaded(call):
    with pytest.raises(ra.RbgError) as ei:
        call()
    assert ei.value.code == ENOTLOADED


def test_every_row_info_and_errors(rb, small, monkeypatch):
    S, T, sym, nxt = small
    rows = np.arange(S.n, dtype=np.uint64)
    fl = FM.FL(S.heads, S.lens)
    if not rb.fl_info()["prepared"]:
        _not_loaded(lambda: rb.fl(rows))
        before = int(rb.info().hbm_bytes)
        assert rb.fl_info() == dict(prepared=False, bytes=0, runs=[0] * 4, shift=[0] * 4, dir_entries=0)
        rb.fl_prepare()
        assert int(rb.info().hbm_bytes) - before >= fl.bytes(int(rb.info().pos_bytes))       # the allocation counts
    mid = int(rb.info().hbm_bytes)
    rb.fl_prepare()                                                                          # idempotent
    assert int(rb.info().hbm_bytes) == mid
    info = rb.fl_info()
    pb = int(rb.info().pos_bytes)
    assert info["prepared"] and info["bytes"] == fl.bytes(pb) and info["runs"] == [fl.runs(c) for c in b"ACGT"] and info["shift"] == [fl.shift(c) for c in b"ACGT"]
    assert info["dir_entries"] == sum((fl.count[c] >> fl.shift(c)) + 2 for c in b"ACGT")
    gs, gn = rb.fl(rows)
    assert (gs == sym).all() and (gn == nxt).all()
    monkeypatch.setenv("RBG_SAM_GRID_CAP", "1")                                              # one workgroup strides over all rows
    gs, gn = rb.fl(rows[::-1].copy())
    monkeypatch.delenv("RBG_SAM_GRID_CAP")
    assert (gs == sym[::-1]).all() and (gn == nxt[::-1]).all()
    assert len(rb.fl(rows[:0])[0]) == 0
    bad = rows[:70].copy()
    bad[33] = S.n                                                                            # a row >= n
    with pytest.raises(ra.RbgError) as ei:
        rb.fl(bad)
    assert ei.value.code == EARG
    gs, gn = rb.fl(rows[:70])                                                                # and the next call is right
    assert (gs == sym[:70]).all() and (gn == nxt[:70]).all()


def test_fl_inverts_lf(rb, small):
    S, T, sym, nxt = small
    rb.fl_prepare()
    rows = np.flatnonzero(np.isin(T.bwt, np.frombuffer(b"ACGT", np.uint8))).astype(np.uint64)
    assert len(rows) == S.n - 1
    lo, hi = rb.LF(rows, rows, T.bwt[rows.astype(np.int64)])
    assert (lo == hi).all()
    gs, gn = rb.fl(lo)
    assert (gs == T.bwt[rows.astype(np.int64)]).all() and (gn == rows).all()


def test_a_replica_prepares_its_own(rb, small):
    S, T, sym, nxt = small
    rb.fl_prepare()
    rows = np.arange(S.n, dtype=np.uint64)
    rep = rb.replicate(0)
    try:
        assert not rep.fl_info()["prepared"]
        _not_loaded(lambda: rep.fl(rows))
        rep.fl_prepare()
        assert rep.fl_info() == rb.fl_info()
        gs, gn = rep.fl(rows)
        assert (gs == sym).all() and (gn == nxt).all()
    finally:
        rep.close()


@pytest.mark.parametrize("layout", [capi.LAYOUT_SLOTS, capi.LAYOUT_RUNS], ids=["slots", "runs"])
def test_rows_across_two_to_the_32(layout):
    rng = np.random.default_rng(611)
    heads, lens, ssa, esa, n = _random_run_index(rng, 400, 50_000_000)
    assert n > 2**32 + 2**30
    fl = FM.FL(heads, lens)
    rows = [0, 1, n - 1, 2**31 - 1, 2**31] + [2**32 + d for d in range(-40, 41)] + [int(v) for v in rng.integers(0, n, 3000)]
    for c in b"ACGT":                                                                        # the first and last row of each base, and rows whose FL crosses
        rows += [fl.F[c], fl.F[c] + fl.count[c] - 1]
    rows = np.array(sorted(set(r for r in rows if 0 <= r < n)), dtype=np.uint64)
    want = [fl.step(int(r)) for r in rows]
    ws, wn = np.array([w[0] for w in want], np.uint8), np.array([w[1] for w in want], np.uint64)
    both = (rows < 2**32) != (wn < 2**32)
    assert (rows >= 2**32).any() and (rows < 2**32).any() and (wn[ws != 0] >= 2**32).any() and both[ws != 0].any() and (ws == 0).any()
    h = _with_layout(layout, lambda: ra.RowBowt.from_runs(heads, lens, ssa, esa, device=0))
    try:
        assert h.info().pos_bytes == 8
        h.fl_prepare()
        assert h.fl_info()["bytes"] == fl.bytes(8)
        gs, gn = h.fl(rows)
        assert (gs == ws).all() and (gn == wn).all()
    finally:
        h.close()
