"""GPU parity of rbg_extend_left_dev (sam_extend.hip k_extend_left) against the text itself: every row of a 2 051-symbol pangenome of five documents is an
item, its read a window of the text left of the row's position with 0 to 10 planted substitutions; the expected record is sam_extend_model.walk_bases fed
from text_ref.TextRef's BWT positions (text[(SA[row] - 1 - t) mod n]: the terminator left of text position 0), no oracle LF involved."""
import numpy as np
import pytest

import rowbowt_amd as ra
import sam_extend_model as XM
from rowbowt_amd import capi
from gpu_common import _with_layout
from synth import SynthIndex
from text_ref import TextRef

pytestmark = pytest.mark.gpu
EARG = -4
KS = (0, 1, 4, 8)


@pytest.fixture(scope="module")
def small():
    S = SynthIndex(L=400, H=5, n_sites=12, seed=41)
    T = TextRef(S.text, S.fm.sa)
    rng = np.random.default_rng(5)
    n = S.n
    seqs, a_, row_, lim_ = [], [], [], []
    for r in range(n):
        l = int(T.sa[r])
        a = (r * 7) % 71                                   # 0 .. 70: neighbouring lanes walk very different distances
        pre = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), max(a - l, 0)).tobytes() + S.text[max(l - a, 0):l].tobytes())
        assert len(pre) == a
        for p in rng.choice(a, min(r % 11, a), replace=False) if a else []:
            pre[p] = ord("ACGT"[("ACGT".index(chr(pre[p])) + 1 + r % 3) % 4]) if chr(pre[p]) in "ACGT" else ord("C")
        if r % 13 == 5 and a > 3:
            pre[a - 3] = ord("N")
        if r % 17 == 3 and a > 6:
            pre[a - 6] = ord(chr(pre[a - 6]).lower())
        seqs.append(bytes(pre) + S.text[l:l + 6].tobytes())
        a_.append(a)
        row_.append(r)
        lim_.append((0, 1, a, a + 5, 1 << 40)[r % 5])
    perm = rng.permutation(n)                              # item j reads sequence perm[j]
    packed, off = ra.pack_reads([seqs[j] for j in np.argsort(perm)])
    items = dict(seq=perm.astype(np.uint32), a=np.array(a_, np.uint32), row=np.array(row_, np.uint64), limit=np.array(lim_, np.uint64))
    want = {}
    for K in KS:
        recs = []
        for r in range(n):
            l = int(T.sa[r])
            recs.append(XM.walk_bases(seqs[r], a_[r], min(a_[r], lim_[r]), K, lambda t: int(S.text[(l - 1 - t) % n])))
        want[K] = recs
    return S, T, packed, off, items, want


@pytest.fixture(scope="module", params=[(capi.LAYOUT_SLOTS, 0), (capi.LAYOUT_RUNS, 0), (capi.LAYOUT_SLOTS, 8), (capi.LAYOUT_RUNS, 8)],
                ids=["slots", "runs", "slots-8-byte", "runs-8-byte"])
def rb(request, small):
    """both layouts at the width the index asks for (4-byte positions) and with 8-byte positions forced: the four instantiations of k_extend_left"""
    S = small[0]
    layout, pos_bytes = request.param
    with capi.default_option(capi.OPT_POS_BYTES, pos_bytes):
        h = _with_layout(layout, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    assert h.info().pos_bytes == (pos_bytes or 4)
    yield h
    h.close()


def _same(got, recs):
    assert len(got) == len(recs)
    for j, (g, x) in enumerate(zip(got, recs)):
        mine = (int(g["ext"]), int(g["nm"]), int(g["score"]), int(g["steps"]), tuple(int(v) for v in g["mis_t"]), tuple(int(v) for v in g["mis_ref"]))
        assert mine == XM.record_tuple(x), (j, mine, XM.record_tuple(x))


def test_inputs_hold_the_cases(small):
    S, T, packed, off, items, want = small
    assert 1900 <= S.n <= 2200 and len(S.doc_starts) == 5
    w = want[4]
    term = [r for r in range(S.n) if w[r]["why"] == "base"]
    assert any(w[r]["steps"] > 0 for r in term) and any(w[r]["steps"] == 0 and items["limit"][r] > 0 and items["a"][r] > 0 for r in term)   # the terminator
    assert int(T.bwt[int(np.flatnonzero(T.sa == 0)[0])]) == 1
    steps = np.array([x["steps"] for x in w])
    assert steps[:64].max() - steps[:64].min() >= 40 and steps.max() == 70                  # one wave, very different walks
    for K in KS:
        assert {x["why"] for x in want[K]} == {"length", "budget", "base"}
        assert max(len(x["mis"]) for x in want[K]) == K
    assert any(len(x["mis"]) > x["nm"] for x in want[8]) and any(x["ext"] == a and a > 20 for x, a in zip(want[8], items["a"]))
    assert {int(v) for v in items["limit"] - np.minimum(items["limit"], items["a"])} > {0}   # limits beyond a


@pytest.mark.parametrize("K", KS)
def test_every_row(rb, small, K):
    S, T, packed, off, items, want = small
    _same(rb.extend_left(packed, off, items["seq"], items["a"], items["row"], items["limit"], K), want[K])


def test_one_workgroup_strides_and_a_replica(rb, small, monkeypatch):
    S, T, packed, off, items, want = small
    monkeypatch.setenv("RBG_SAM_GRID_CAP", "1")
    _same(rb.extend_left(packed, off, items["seq"], items["a"], items["row"], items["limit"], 4), want[4])
    monkeypatch.delenv("RBG_SAM_GRID_CAP")
    rep = rb.replicate(0)
    try:
        _same(rep.extend_left(packed, off, items["seq"], items["a"], items["row"], items["limit"], 8), want[8])
    finally:
        rep.close()
    sub = slice(0, 65)                                     # a wave and one lane
    _same(rb.extend_left(packed, off, items["seq"][sub], items["a"][sub], items["row"][sub], items["limit"][sub], 1), want[1][sub])
    assert len(rb.extend_left(packed, off, items["seq"][:0], items["a"][:0], items["row"][:0], items["limit"][:0], 1)) == 0


def test_errors(rb, small):
    S, T, packed, off, items, want = small
    args = lambda **kw: [kw.get(k, items[k][:70]) for k in ("seq", "a", "row", "limit")]
    with pytest.raises(ra.RbgError) as ei:
        rb.extend_left(packed, off, *args(), 9)
    assert ei.value.code == EARG
    N = len(off) - 1
    for bad in (dict(seq=np.where(np.arange(70) == 33, N, items["seq"][:70]).astype(np.uint32)),           # a sequence index >= N
                dict(row=np.where(np.arange(70) == 7, S.n, items["row"][:70]).astype(np.uint64)),           # a row >= n
                dict(a=np.where(np.arange(70) == 69, 5000, items["a"][:70]).astype(np.uint32))):            # a beyond its sequence
        with pytest.raises(ra.RbgError) as ei:
            rb.extend_left(packed, off, *args(**bad), 4)
        assert ei.value.code == EARG
    _same(rb.extend_left(packed, off, *args(), 4), want[4][:70])                                            # and the next call is right
