"""The model of the left extension (tests/sam_extend_model.py: what rbg_extend_left_dev and rbg_align_sam_extend must produce) against the text itself, and the
shared inputs of the GPU tests (tests/sam_extend_cases.py) against the list of line kinds they are meant to hold.  No GPU."""
import numpy as np
import pytest

import rowbowt_amd as ra
import sam_extend_cases as XC
import sam_extend_model as XM
import sam_model as SAM

KS = (0, 1, 4, 8)


def _direct(text, l, s, a, L, K):
    """the rule evaluated on the bytes text[l - L : l] and s[a - L : a] alone"""
    return XM.walk_bases(s, a, L, K, lambda t: int(text[l - 1 - t]) if l - 1 - t >= 0 else None)


@pytest.mark.parametrize("K", KS)
def test_model_against_the_text(K):
    S, o = XC.toy()
    text = S.text
    checked = 0
    for (_, q), recs in zip(XC.reads(S), XC.records(K)):
        if recs == [None]:
            continue
        for (lo, hi, k, a, b, rev), j, l, dn, offs, x in recs:
            s = SAM.revcomp(q) if rev else q
            assert text[l:l + b - a].tobytes() == s[a:b]                                   # the seed itself, at the line's location
            assert int(S.fm.sa[hi - (j - 1)]) == l                                         # line j of [lo, hi] is row hi - (j - 1)
            e = x["ext"]
            want = _direct(text, l, s, a, min(a, offs), K)
            assert {f: x[f] for f in ("ext", "nm", "score", "steps", "mis", "why")} == want, (q, j)
            ref, mine = text[l - e:l].tobytes(), s[a - e:a]
            diff = [(e - 1 - u, ref[u]) for u in range(e) if ref[u] != mine[u]]
            assert sorted(diff) == x["mis"][:x["nm"]] and len(diff) == x["nm"]              # exactly the recorded mismatches inside the extension
            assert e == 0 or ref[0] == mine[0]                                              # it ends on a match
            assert x["score"] == e - 5 * x["nm"] >= 0
            # MD re-expands to the reference bytes of [a - e, b)
            md, out, pos, num = XM.md(x, b - a), bytearray(), a - e, b""
            for ch in md + b"$":
                if chr(ch).isdigit():
                    num += bytes([ch])
                    continue
                out += s[pos:pos + int(num)]
                pos += int(num)
                num = b""
                if ch != ord("$"):
                    out.append(ch)
                    pos += 1
            assert bytes(out) == text[l - e:l + b - a].tobytes() and pos == b and md[:1].isdigit() and md[-1:].isdigit()
            checked += 1
    assert checked >= 150


def test_shared_inputs_hold_every_kind_of_line():
    """so that no GPU test passes on an empty case.  A walk ended by the terminator cannot happen on a line -- document 0 starts at text position 0, and the
    limit offs ends the walk there first --: that kind is among the ITEMS of the primitive's test, asserted below from the same model"""
    seen = set().union(*(XC.kinds(K) for K in KS))
    assert seen >= {"e = a", "0 < e < a by the budget", "cut by offs", "e = 0, a > 0", "trimmed a taken mismatch", "secondary lines of different nm", "forward",
                    "reverse", "N in the flank", "a = 0", "unmapped"}, seen
    assert {"e = a", "cut by offs", "trimmed a taken mismatch", "secondary lines of different nm", "N in the flank"} <= XC.kinds(4)
    assert "0 < e < a by the budget" in XC.kinds(1) and XC.kinds(0) >= {"e = 0, a > 0", "forward", "reverse"}
    S, o = XC.toy()
    row0 = int(np.flatnonzero(S.fm.sa == 0)[0])                                             # the row whose BWT is the terminator
    assert o.access(row0) == 1
    q = S.text[:40].tobytes()
    x = XM.extend(o, b"ACGTACGT" + q, 8, row0, 5, 4)
    assert x["why"] == "base" and x["steps"] == 0 and x["ext"] == 0
    row3 = int(np.flatnonzero(S.fm.sa == 3)[0])
    x = XM.extend(o, b"ACGTA" + S.text[:43].tobytes(), 8, row3, 100, 4)                     # three bases, then the terminator
    assert x["why"] == "base" and x["steps"] == 3 and x["ext"] == 3


def test_abi_surface():
    L = ra.lib()
    for f in ("rbg_align_sam_extend", "rbg_extend_left_dev"):
        assert hasattr(L, f), f
    assert L.rbg_align_sam_extend(None, None, None, None, None, None, None, None, None, 0, 20, 16, 0, 4, None, None) == -4     # RBG_EARG
    assert L.rbg_extend_left_dev(None, None, None, 0, None, None, None, None, 0, 4, None, None) == -4
    assert callable(ra.RowBowt.align_sam_extend) and callable(ra.RowBowt.extend_left)
    from rowbowt_amd import capi
    assert capi.EXTEND.itemsize == 56 and capi.SAM_MAX_MISMATCH == XM.MAX_MISMATCH == 8
