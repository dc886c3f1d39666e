"""The FL model (tests/fl_model.py: what rbg_fl_dev and rbg_extend_right_dev must produce) against the text and its suffix array alone (text_ref.TextRef): no
oracle, no library answers.  The ABI surface of the new entry points.  No GPU."""
import numpy as np
import pytest

import fl_model as FM
import rowbowt_amd as ra
from synth import SynthIndex
from text_ref import TextRef


@pytest.fixture(scope="module")
def small():
    S = SynthIndex(L=400, H=5, n_sites=12, seed=41)
    return S, TextRef(S.text, S.fm.sa), FM.FL(S.heads, S.lens)


def test_every_row_against_the_text(small):
    S, T, fl = small
    n = S.n
    assert fl.n == n == 2051
    nobase = 0
    for row in range(n):
        p = int(T.sa[row])
        c = int(T.text[p])
        sym, nxt = fl.step(row)
        if c in b"ACGT":
            assert (sym, nxt) == (c, int(T.isa[(p + 1) % n])), row
        else:
            assert (sym, nxt) == (0, FM.NONE), row
            nobase += 1
    assert nobase == 1                                       # the terminator's row (this text's separators are runs of A)
    for c in b"ACGT":
        assert fl.F[c] == int(T.C[c]) and fl.count[c] == int(T.C[c + 1] - T.C[c])


def test_fl_inverts_lf(small):
    S, T, fl = small
    for row in range(S.n):
        c = int(T.bwt[row])
        if c in b"ACGT":
            lo, hi = T.lf([row], [row], [c])
            assert int(lo[0]) == int(hi[0]) and fl.step(int(lo[0])) == (c, row)


def test_right_walk_against_the_text(small):
    S, T, fl = small
    n, text = S.n, S.text
    rng = np.random.default_rng(3)
    whys = set()
    near_end = {int(T.isa[n - 1 - d]) for d in range(4)}    # rows whose 8 skip steps meet the terminator
    for row in sorted(set(range(0, n, 3)) | near_end):
        l = int(T.sa[row])
        skip, m = (8 if row in near_end else row % 9), 40
        right = bytearray(text[l + skip:l + skip + m].tobytes())
        right += bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), m - len(right)).tobytes())
        for p in rng.choice(m, row % 5, replace=False):
            right[p] = ord("ACGT"[("ACGT".index(chr(right[p])) + 1) % 4]) if chr(right[p]) in "ACGT" else ord("C")
        s = bytes(text[l:l + skip].tobytes()).ljust(skip, b"A") + bytes(right)
        for K in (0, 2, 8):
            got = FM.extend_right(fl, s, skip, row, skip, 1 << 40, K)
            if l + skip >= n:                                # the skip meets the terminator's row
                assert got["why"] == "skip" and got["ext"] == 0
            else:
                want = FM.walk_right(s, skip, m, K, lambda t: int(text[l + skip + t]) if l + skip + t < n else None)
                assert got == want, (row, K)
            whys.add(got["why"])
    assert whys >= {"length", "budget", "base", "skip"}


def test_md_of_both_flanks():
    x = dict(ext=7, nm=1, score=2, steps=7, mis=[(2, ord("C"))])
    y = dict(ext=9, nm=2, score=-1, steps=9, mis=[(0, ord("G")), (5, ord("T")), (8, ord("A"))])
    assert FM.md_both(x, y, 20) == b"4C22G4T3"
    assert FM.md_both(dict(ext=0, nm=0, mis=[]), dict(ext=0, nm=0, mis=[]), 31) == b"31"
    assert FM.md_both(dict(ext=0, nm=0, mis=[]), dict(ext=4, nm=1, mis=[(1, ord("A"))]), 10) == b"11A2"


def test_abi_surface():
    L = ra.lib()
    for f in ("rbg_fl_prepare", "rbg_fl_info", "rbg_fl_dev", "rbg_extend_right_dev", "rbg_align_sam_extend_both"):
        assert hasattr(L, f), f
    assert L.rbg_fl_prepare(None) == -4                       # RBG_EARG
    assert L.rbg_fl_info(None, None) == -4
    assert L.rbg_fl_dev(None, None, 0, None, None, None) == -4
    assert L.rbg_extend_right_dev(None, None, None, 0, None, None, None, None, None, 0, 4, None, None) == -4
    assert L.rbg_align_sam_extend_both(None, None, None, None, None, None, None, None, None, 0, 20, 16, 0, 4, None, None) == -4
    for m in ("fl_prepare", "fl_info", "fl", "extend_right", "align_sam_extend"):
        assert callable(getattr(ra.RowBowt, m)), m
