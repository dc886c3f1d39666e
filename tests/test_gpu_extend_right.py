"""GPU parity of rbg_extend_right_dev (fl_extend.hip k_extend_right) against the text itself: every row of a 2 051-symbol pangenome of five documents is an
item, its read the text window right of the row's position (the skipped bases, then the compared ones) with 0 to 10 planted substitutions; the expected
record is fl_model.walk_right -- sam_extend_model.walk_bases with s[b + t] -- fed from text[(SA[row] + skip + t) mod n], no FL model and no oracle involved.
This text's separators are runs of A, which are bases: a walk ends ON a separator by its limit or its budget there, on the terminator by the byte."""
import numpy as np
import pytest

import fl_model as FM
import rowbowt_amd as ra
import sam_extend_model as XM
from rowbowt_amd import capi
from gpu_common import _with_layout
from synth import SynthIndex
from text_ref import TextRef

pytestmark = pytest.mark.gpu
EARG, ENOTLOADED = -4, -6
KS = (0, 1, 4, 8)
ZERO = dict(ext=0, nm=0, score=0, steps=0, mis=[], why="skip")


@pytest.fixture(scope="module")
def small():
    S = SynthIndex(L=400, H=5, n_sites=12, seed=41)
    T = TextRef(S.text, S.fm.sa)
    rng = np.random.default_rng(6)
    n, text = S.n, S.text
    seqs, b_, row_, skip_, lim_ = [], [], [], [], []
    for r in range(n):
        l = int(T.sa[r])
        skip = (r * 7) % 71                                # 0 .. 70 within a wave: neighbouring lanes cross seeds of very different lengths
        tail = 10 + (r * 11) % 61                          # m - b: 10 .. 70
        body = bytearray(text[l:l + skip + tail].tobytes())
        body += bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), skip + tail - len(body)).tobytes())
        for p in rng.choice(tail, min(r % 11, tail), replace=False):
            q = skip + int(p)
            body[q] = ord("ACGT"[("ACGT".index(chr(body[q])) + 1 + r % 3) % 4]) if chr(body[q]) in "ACGT" else ord("C")
        if r % 13 == 5:
            body[skip + 3] = ord("N")
        if r % 17 == 3:
            body[skip + 6] = ord(chr(body[skip + 6]).lower())
        seqs.append(bytes(body))
        b_.append(skip)
        row_.append(r)
        skip_.append(skip)
        lim_.append((0, 1, tail, tail + 5, 1 << 40)[r % 5])
    perm = rng.permutation(n)                              # item j reads sequence perm[j]
    packed, off = ra.pack_reads([seqs[j] for j in np.argsort(perm)])
    items = dict(seq=perm.astype(np.uint32), b=np.array(b_, np.uint32), row=np.array(row_, np.uint64), skip=np.array(skip_, np.uint32),
                 limit=np.array(lim_, np.uint64))
    want = {}
    for K in KS:
        recs = []
        for r in range(n):
            l, skip = int(T.sa[r]), skip_[r]
            if any(int(text[(l + s) % n]) not in b"ACGT" for s in range(skip)):
                recs.append(ZERO)                          # the skip meets a row without a base
                continue
            m = len(seqs[r])
            recs.append(FM.walk_right(seqs[r], skip, min(m - skip, lim_[r]), K, lambda t: int(text[(l + skip + t) % n])))
        want[K] = recs
    return S, T, packed, off, items, want


@pytest.fixture(scope="module", params=[(capi.LAYOUT_SLOTS, 0), (capi.LAYOUT_RUNS, 0), (capi.LAYOUT_SLOTS, 8), (capi.LAYOUT_RUNS, 8)],
                ids=["slots", "runs", "slots-8-byte", "runs-8-byte"])
def rb(request, small):
    S = small[0]
    layout, pos_bytes = request.param
    with capi.default_option(capi.OPT_POS_BYTES, pos_bytes):
        h = _with_layout(layout, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    assert h.info().pos_bytes == (pos_bytes or 4)
    h.fl_prepare()
    yield h
    h.close()


def _same(got, recs):
    assert len(got) == len(recs)
    for j, (g, x) in enumerate(zip(got, recs)):
        mine = (int(g["ext"]), int(g["nm"]), int(g["score"]), int(g["steps"]), tuple(int(v) for v in g["mis_t"]), tuple(int(v) for v in g["mis_ref"]))
        assert mine == XM.record_tuple(x), (j, mine, XM.record_tuple(x))


def _args(items, sub=slice(None), **kw):
    return [kw.get(k, items[k][sub]) for k in ("seq", "b", "row", "skip", "limit")]


def test_inputs_hold_the_cases(small):
    S, T, packed, off, items, want = small
    n, unit = S.n, S.L + S.pad
    assert 1900 <= n <= 2200 and len(S.doc_starts) == 5
    for K in KS:
        assert {x["why"] for x in want[K]} == {"length", "budget", "base", "skip"}            # all three endings, and a skip that meets "no base"
        assert max(len(x["mis"]) for x in want[K]) == K
    w = want[4]
    ends = [(int(T.sa[r]) + int(items["skip"][r]) + x["steps"]) for r, x in enumerate(w)]     # the text position where the walk stopped
    assert any(x["why"] == "base" and e == n - 1 and x["steps"] > 0 for x, e in zip(w, ends))                     # ... on the terminator
    assert any(x["why"] in ("length", "budget") and x["steps"] > 0 and e < n - 1 and e % unit >= S.L for x, e in zip(w, ends))   # ... on a separator
    steps = np.array([x["steps"] for x in w])
    assert steps[:64].max() - steps[:64].min() >= 40
    assert int(items["skip"][:64].max()) - int(items["skip"][:64].min()) >= 60
    assert any(len(x["mis"]) > x["nm"] for x in want[8]) and any(x["ext"] > 40 and x["nm"] > 0 for x in want[8])     # trimmed mismatches; long extensions
    assert {int(v) for v in items["limit"]} >= {0, 1, 1 << 40}


@pytest.mark.parametrize("K", KS)
def test_every_row(rb, small, K):
    S, T, packed, off, items, want = small
    _same(rb.extend_right(packed, off, *_args(items), K), want[K])


def test_one_workgroup_strides_and_a_replica(rb, small, monkeypatch):
    S, T, packed, off, items, want = small
    monkeypatch.setenv("RBG_SAM_GRID_CAP", "1")
    _same(rb.extend_right(packed, off, *_args(items), 4), want[4])
    monkeypatch.delenv("RBG_SAM_GRID_CAP")
    rep = rb.replicate(0)
    try:
        with pytest.raises(ra.RbgError) as ei:
            rep.extend_right(packed, off, *_args(items), 8)
        assert ei.value.code == ENOTLOADED
        rep.fl_prepare()
        _same(rep.extend_right(packed, off, *_args(items), 8), want[8])
    finally:
        rep.close()
    sub = slice(0, 65)                                     # a wave and one lane
    _same(rb.extend_right(packed, off, *_args(items, sub), 1), want[1][sub])
    assert len(rb.extend_right(packed, off, *_args(items, slice(0, 0)), 1)) == 0


def test_errors(rb, small):
    S, T, packed, off, items, want = small
    sub = slice(0, 70)
    with pytest.raises(ra.RbgError) as ei:
        rb.extend_right(packed, off, *_args(items, sub), 9)
    assert ei.value.code == EARG
    N = len(off) - 1
    at = lambda j, v, a, t: np.where(np.arange(70) == j, v, a[:70]).astype(t)
    for bad in (dict(seq=at(33, N, items["seq"], np.uint32)),                                 # a sequence index >= N
                dict(row=at(7, S.n, items["row"], np.uint64)),                                # a row >= n
                dict(b=at(69, 5000, items["b"], np.uint32)),                                  # b beyond its sequence
                dict(skip=at(12, int(items["b"][12]) + 1, items["skip"], np.uint32))):        # skip > b
        with pytest.raises(ra.RbgError) as ei:
            rb.extend_right(packed, off, *_args(items, sub, **bad), 4)
        assert ei.value.code == EARG
    _same(rb.extend_right(packed, off, *_args(items, sub), 4), want[4][:70])                  # and the next call is right
