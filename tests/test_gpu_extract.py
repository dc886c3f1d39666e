"""GPU parity of rbg_extract_dev and rbg_extract (extract.hip k_extract) against the text itself, byte for byte: every position of two texts (tests/isa_model.py:
the 2 051-symbol pangenome and the hand-built text with '#', a run of N and a document that starts with N) with every length of isa_model.LENS, on both
layouts at 4-byte and forced 8-byte positions.  Expected: text[p:] up to the first byte that is no base, then zeros (isa_model.expected; no library call)."""
import numpy as np
import pytest
import torch

import isa_model as IM
import rowbowt_amd as ra
from rowbowt_amd import capi
from gpu_common import _with_layout

pytestmark = pytest.mark.gpu
EARG = -4


@pytest.fixture(scope="module", params=["synth", "hand"])
def text(request):
    return IM.synth_text() if request.param == "synth" else IM.hand_text()


@pytest.fixture(scope="module", params=[(capi.LAYOUT_SLOTS, 0), (capi.LAYOUT_RUNS, 0), (capi.LAYOUT_SLOTS, 8), (capi.LAYOUT_RUNS, 8)],
                ids=["slots", "runs", "slots-8-byte", "runs-8-byte"])
def rb(request, text):
    layout, pos_bytes = request.param
    with capi.default_option(capi.OPT_POS_BYTES, pos_bytes):
        h = _with_layout(layout, lambda: ra.RowBowt.from_runs(text.heads, text.lens, text.ssa, text.esa, device=0))
    h.extract_prepare()
    yield h
    h.close()


@pytest.fixture(scope="module")
def items(text):
    """every (position, length) laid out with gaps of 1 .. 17 bytes between the items: (pos, len, out_off, the expected buffer over 0xA5, the expected got)"""
    T = text
    pos, length, off, want_got = [], [], [], []
    at = 3
    for p in range(T.n):
        for L in IM.LENS:
            pos.append(p), length.append(L), off.append(at)
            at += L + 1 + (len(off) % 17)
    total = at + 5
    want = np.full(total, 0xA5, np.uint8)
    for p, L, o in zip(pos, length, off):
        b, g = IM.expected(T.tb, p, L)
        want[o:o + L] = np.frombuffer(b, np.uint8)
        want_got.append(g)
    off = np.array(off, np.uint64)
    assert set((off % 16).tolist()) == set(range(16)) and set((off[np.array(length) > 20] % 16).tolist()) == set(range(16))
    gaps = off[1:] - (off[:-1] + np.array(length[:-1], np.uint64))
    assert set(gaps.tolist()) == set(range(1, 18))
    return np.array(pos, np.uint64), np.array(length, np.uint32), off, want, np.array(want_got, np.uint32)


def _run_dev(rb, pos, length, off, total):
    with torch.cuda.device(int(rb.info().device)):
        dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()
        d_out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
        d_got = torch.full((max(len(pos), 1),), -6, dtype=torch.int32, device="cuda")
        rb.extract_dev(dev(pos, np.int64), dev(length, np.int32), dev(off, np.int64), d_out, d_got)
        return d_out.cpu().numpy(), d_got.cpu().numpy().view(np.uint32)[:len(pos)]


def test_every_position_and_length_on_guarded_output(rb, items, monkeypatch):
    pos, length, off, want, want_got = items
    out, got = _run_dev(rb, pos, length, off, len(want))
    assert (got == want_got).all()
    bad = np.flatnonzero(out != want)
    assert len(bad) == 0, (bad[:5], out[bad[:5]], want[bad[:5]])                             # exactly len bytes per item: the 0xA5 between them stays
    monkeypatch.setenv("RBG_SAM_GRID_CAP", "1")                                              # one workgroup strides over a reversed stretch
    sub = slice(None, 3000)
    out1, got1 = _run_dev(rb, pos[sub][::-1].copy(), length[sub][::-1].copy(), off[sub][::-1].copy(), len(want))
    monkeypatch.delenv("RBG_SAM_GRID_CAP")
    assert (got1 == want_got[sub][::-1]).all()
    end = int(off[sub][-1]) + int(length[sub][-1])
    assert (out1[:end] == want[:end]).all() and (out1[end:] == 0xA5).all()


def test_a_position_beyond_the_text_is_an_error_and_the_next_call_is_right(rb, items, text):
    pos, length, off, want, want_got = items
    sub = slice(8 * 40, 8 * 40 + 70)
    bad = pos[sub].copy()
    bad[33] = text.n
    with pytest.raises(ra.RbgError) as ei:
        _run_dev(rb, bad, length[sub], off[sub], len(want))
    assert ei.value.code == EARG
    out, got = _run_dev(rb, pos[sub], length[sub], off[sub], len(want))
    assert (got == want_got[sub]).all()
    lo, hi = int(off[sub][0]), int(off[sub][-1]) + int(length[sub][-1])
    assert (out[lo:hi] == want[lo:hi]).all() and (out[:lo] == 0xA5).all() and (out[hi:] == 0xA5).all()
    with pytest.raises(ra.RbgError) as ei:
        rb.extract(np.array([3, text.n], np.uint64), np.array([5, 5], np.uint64))
    assert ei.value.code == EARG


def _intervals(T):
    """(pos, len) that end at a separator, inside the run of N, at the terminator and past n; the whole text as one interval; empty ones"""
    tb, n = T.tb, T.n
    iv = [(0, n), (0, n + 50), (n - 30, 30), (n - 30, 29), (n - 30, 400), (n - 1, 1), (n - 1, 0), (5, 0), (0, 1)]
    for c in (b"#", b"N", b"NNNNN"):
        at = tb.find(c)
        if at >= 0:
            iv += [(at - 40, 40), (at - 40, 41), (at - 40, 100), (at, 10), (at + len(c), 300), (at + len(c) - 1, 20)]
    if T.doc_starts:
        iv += [(s, e - s) for s, e in zip(T.doc_starts, list(T.doc_starts[1:]) + [n])]
    return np.array([p for p, _ in iv], np.uint64), np.array([l for _, l in iv], np.uint64)


def test_host_call_does_not_depend_on_the_chunk(rb, text):
    T = text
    pos, length = _intervals(T)
    want = [IM.expected(T.tb, int(p), int(l)) for p, l in zip(pos, length)]
    if T is IM.hand_text():
        stops = {T.tb[int(p) + g] for (b, g), p, l in zip(want, pos, length) if g < l and int(p) + g < T.n}
        assert stops == {1, ord("#"), ord("N")}
    assert any(int(p) + int(l) > T.n for p, l in zip(pos, length)) and any(g == T.n - 1 for _, g in want) == (T is IM.synth_text())
    results = []
    for chunk in (None, 7, 1):
        if chunk is None:
            assert capi.get_default_option(capi.OPT_EXTRACT_CHUNK) == 128
            results.append(rb.extract(pos, length))
        else:
            with capi.default_option(capi.OPT_EXTRACT_CHUNK, chunk):
                results.append(rb.extract(pos, length))
    for text_out, got in results:
        assert got.tolist() == [g for _, g in want]
        assert text_out == b"".join(b for b, _ in want)
    one, g = rb.extract(7, 33)                                                               # a single interval: (bytes, int)
    assert (one, g) == IM.expected(T.tb, 7, 33)
    with pytest.raises(ra.RbgError) as ei:
        capi.set_default_option(capi.OPT_EXTRACT_CHUNK, 0)
    assert ei.value.code == EARG


def test_fl_chained_from_isa_agrees_with_extract(rb, text):
    T = text
    pos = np.arange(T.n, dtype=np.uint64)
    L = 17
    rows = rb.isa(pos)
    out = np.zeros((T.n, L), np.uint8)
    live = np.ones(T.n, bool)
    for t in range(L):
        idx = np.flatnonzero(live)
        sym, nxt = rb.fl(rows[idx])
        out[idx, t] = sym
        rows[idx] = nxt
        live[idx[sym == 0]] = False
    text_out, got = rb.extract(pos, np.full(T.n, L, np.uint64))
    assert np.frombuffer(text_out, np.uint8).reshape(T.n, L).tolist() == out.tolist()
    assert (got == (out != 0).sum(axis=1)).all()
