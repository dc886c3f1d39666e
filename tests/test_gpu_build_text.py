"""rbg_build_from_text / rbg_convert_text (capi/build_text.ipp) on the GPU: the handle RowBowt.from_text builds from a text holds, array for array
(rbg_host_array), what RowBowt.from_runs builds from the naive run arrays of the same text, on both layouts, and passes the sweep drivers of
tests/sweeps.py as they are and in full on both texts: every ACGT string of lengths 1-9, every text window of lengths 10-24, the long windows and the
substituted windows (A) -- on docs() those windows run across '#', '##' and the runs of N, which the engine matches as the bytes they are --, LF at every
row (B), phi at every text position (C).

Cache identity: the cache file has no field that varies by build (rbg_host.hpp write_flat: arrays, lengths and a checksum of them), so rbg_convert_text's
file is compared BYTE FOR BYTE with rbg_convert_runs_markers' file from the naive arrays and the same docs text."""
import numpy as np
import pytest

import extract_wide_cases as EW
import isa_model as IM
import rowbowt_amd as ra
import sweeps
from rowbowt_amd import capi
from gpu_common import _with_layout

pytestmark = pytest.mark.gpu
ENODEV, EARG, ENOMEM = -3, -4, -5
ARRAYS = (capi.ARR_RUN_HEADS, capi.ARR_RUN_START, capi.ARR_SAMPLES_LAST, capi.ARR_PRED_POS, capi.ARR_PHI_BASE)
_made = {}


def _text(name):
    if name not in _made:
        T = IM.synth_text() if name == "synth" else EW.docs()
        X = sweeps.Index(T.text, T.sa)
        symbols = list(b"ACGT\x01N#")
        _made[name] = dict(T=T, X=X, A=sweeps.sweep_a(X.ref), B=sweeps.sweep_b(X.ref, symbols), C=sweeps.sweep_c(X.ref))
    return _made[name]


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    _made.clear()


@pytest.mark.parametrize("layout", [capi.LAYOUT_SLOTS, capi.LAYOUT_RUNS], ids=["slots", "runs"])
@pytest.mark.parametrize("name", ["synth", "docs"])
def test_from_text_is_from_runs_and_passes_the_sweeps(name, layout):
    M = _text(name)
    T, X = M["T"], M["X"]
    rb = _with_layout(layout, lambda: ra.RowBowt.from_text(T.tb, device=0))
    want = _with_layout(layout, lambda: ra.RowBowt.from_runs(T.heads, T.lens, T.ssa, T.esa, device=0))
    try:
        info = rb.info()
        assert info.n == T.n and info.r == len(T.heads) and info.has_tsa == 1 and info.rank_layout == layout
        assert capi.sa_info()["n"] == T.n
        for which in ARRAYS:
            assert (rb.host_array(which) == want.host_array(which)).all(), which
        cfg = "%s from_text (layout %d)" % (name, layout)
        sweeps.run_sweep_a(cfg, rb, M["A"])
        sweeps.run_sweep_b(cfg, rb, M["B"])
        sweeps.run_sweep_c(cfg, rb, M["C"])
    finally:
        rb.close(), want.close()


def test_without_sa_no_samples_are_kept():
    T = IM.synth_text()
    rb = ra.RowBowt.from_text(T.text, sa=False, device=0)
    assert rb.info().has_tsa == 0 and rb.info().n == T.n
    seqs, off = ra.pack_reads([T.tb[100:140]])
    lo, hi = rb.find_range(seqs, off)
    assert int(hi[0]) >= int(lo[0])
    rb.close()


def test_cache_file_is_the_one_from_the_naive_arrays(tmp_path):
    T = EW.docs()
    docs_text = "".join(f"{n} {s}\n" for n, s in zip(T.doc_names, T.doc_starts))
    a, b = tmp_path / "text.rbgpu", tmp_path / "runs.rbgpu"
    capi.convert_text(T.tb, a, docs_text=docs_text)
    capi.convert_runs(T.heads, T.lens, T.ssa, T.esa, out_path=b, docs_text=docs_text)
    assert a.read_bytes() == b.read_bytes()
    capi.convert_text(T.tb, a, sa=False)
    capi.convert_runs(T.heads, T.lens, out_path=b)
    assert a.read_bytes() == b.read_bytes()


def test_error_codes():
    L = ra.lib()
    T = IM.synth_text()
    h = capi.VP()
    assert L.rbg_build_from_text(capi._p(T.text), T.n, 1, capi.DEVICE_NONE, capi.C.byref(h)) == ENODEV and not h.value
    assert L.rbg_convert_text(capi._p(T.text), T.n, None, 1, capi.DEVICE_NONE, b"/dev/null") == ENODEV
    # a text whose build cannot fit the device, with no text behind the pointer: refused before the text is touched
    assert L.rbg_build_from_text(None, 1 << 40, 1, 0, capi.C.byref(h)) == ENOMEM and not h.value
    assert L.rbg_convert_text(None, 1 << 40, None, 1, 0, b"/dev/null") == ENOMEM
    assert L.rbg_build_from_text(None, 100, 1, 0, capi.C.byref(h)) == EARG
    assert L.rbg_build_from_text(capi._p(T.text), 0, 1, 0, capi.C.byref(h)) == EARG
    bad = T.text.copy()
    bad[5] = 1                                                                              # the smallest byte twice
    assert L.rbg_build_from_text(capi._p(bad), T.n, 1, 0, capi.C.byref(h)) == EARG and not h.value
