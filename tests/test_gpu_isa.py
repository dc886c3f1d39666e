"""GPU parity of rbg_isa_dev (extract.hip k_isa_rows over the ISA sample of rbg_extract_prepare) against the text itself: at every position of two texts
row = ISA[p] (the inverse of a naive suffix array; no oracle) -- the 2 051-symbol pangenome of the FL tests and a text built by hand with '#' separators, a
run of five N and a document that starts with N (tests/isa_model.py) --, on both layouts at 4-byte and forced 8-byte positions; rbg_extract_info against the
model's numbers."""
import numpy as np
import pytest

import isa_model as IM
import rowbowt_amd as ra
from rowbowt_amd import capi
from gpu_common import _with_layout

pytestmark = pytest.mark.gpu
EARG, ENOTLOADED = -4, -6
UNPREPARED = dict(prepared=False, bytes=0, samples=0, shift=0, dir_entries=0, second_kind=0, max_gap=0, build_us=0)


@pytest.fixture(scope="module", params=["synth", "hand"])
def text(request):
    return IM.synth_text() if request.param == "synth" else IM.hand_text()


@pytest.fixture(scope="module", params=[(capi.LAYOUT_SLOTS, 0), (capi.LAYOUT_RUNS, 0), (capi.LAYOUT_SLOTS, 8), (capi.LAYOUT_RUNS, 8)],
                ids=["slots", "runs", "slots-8-byte", "runs-8-byte"])
def rb(request, text):
    layout, pos_bytes = request.param
    with capi.default_option(capi.OPT_POS_BYTES, pos_bytes):
        h = _with_layout(layout, lambda: ra.RowBowt.from_runs(text.heads, text.lens, text.ssa, text.esa, device=0))
    assert h.info().pos_bytes == (pos_bytes or 4)
    yield h
    h.close()


def _not_loaded(call):
    with pytest.raises(ra.RbgError) as ei:
        call()
    assert ei.value.code == ENOTLOADED


def test_every_position_info_and_errors(rb, text, monkeypatch):
    T = text
    M = T.model()
    pos = np.arange(T.n, dtype=np.uint64)
    want = T.isa.astype(np.uint64)
    pb = int(rb.info().pos_bytes)
    if not rb.extract_info()["prepared"]:
        _not_loaded(lambda: rb.isa(pos))
        _not_loaded(lambda: rb.extract(0, 4))
        assert rb.extract_info() == UNPREPARED
        before = int(rb.info().hbm_bytes)
        rb.extract_prepare()
        assert int(rb.info().hbm_bytes) - before >= M.bytes(pb)                              # the allocation counts
    assert rb.fl_info()["prepared"]                                                          # extract_prepare ran fl_prepare
    mid = int(rb.info().hbm_bytes)
    rb.extract_prepare()                                                                     # idempotent
    assert int(rb.info().hbm_bytes) == mid
    info = rb.extract_info()
    assert info.pop("build_us") >= 0
    assert info == dict(prepared=True, bytes=M.bytes(pb), samples=M.samples, shift=M.shift, dir_entries=M.dir_entries, second_kind=M.second_kind,
                        max_gap=M.max_gap)
    assert (rb.isa(pos) == want).all()
    monkeypatch.setenv("RBG_SAM_GRID_CAP", "1")                                              # one workgroup strides over all positions, reversed
    got = rb.isa(pos[::-1].copy())
    monkeypatch.delenv("RBG_SAM_GRID_CAP")
    assert (got == want[::-1]).all()
    assert len(rb.isa(pos[:0])) == 0                                                         # M = 0
    assert rb.extract(pos[:0], pos[:0])[0] == b""
    bad = pos[:70].copy()
    bad[33] = T.n                                                                            # a position >= n in the middle of 70
    with pytest.raises(ra.RbgError) as ei:
        rb.isa(bad)
    assert ei.value.code == EARG
    assert (rb.isa(pos[:70]) == want[:70]).all()                                             # and the next call is right


def test_fl_prepared_first_counts_only_the_sample(text):
    T = text
    M = T.model()
    h = ra.RowBowt.from_runs(T.heads, T.lens, T.ssa, T.esa, device=0)
    try:
        h.fl_prepare()
        before = int(h.info().hbm_bytes)
        h.extract_prepare()
        grown = int(h.info().hbm_bytes) - before
        assert M.bytes(4) <= grown < M.bytes(4) + 2 * 64 * 1024                              # one allocation, rounded up
    finally:
        h.close()


def test_a_replica_prepares_its_own(rb, text):
    T = text
    rb.extract_prepare()
    pos = np.arange(T.n, dtype=np.uint64)
    rep = rb.replicate(0)
    try:
        assert rep.extract_info() == UNPREPARED
        _not_loaded(lambda: rep.isa(pos))
        rep.extract_prepare()
        a, b = rep.extract_info(), rb.extract_info()
        a.pop("build_us"), b.pop("build_us")
        assert a == b
        assert (rep.isa(pos) == T.isa.astype(np.uint64)).all()
    finally:
        rep.close()


def test_without_toehold_samples_there_is_nothing_to_prepare(text):
    h = ra.RowBowt.from_runs(text.heads, text.lens, device=0)
    try:
        _not_loaded(h.extract_prepare)
    finally:
        h.close()
