"""GPU parity of rbg_align_sam_extend_both (fl_extend.hip, capi/sam.ipp) against tests/fl_model.py: the whole text, byte for byte.  The reads are
tests/sam_extend_cases.py's plus windows with substitutions planted RIGHT of the seed; a model-only test asserts which kinds of line they hold."""
import functools
import re

import numpy as np
import pytest

import fl_model as FM
import rowbowt_amd as ra
import sam_extend_cases as XC
import sam_extend_model as XM
import sam_model as SAM
from rowbowt_amd import capi
from gpu_common import _with_layout

pytestmark = pytest.mark.gpu
ENOTLOADED = -6
KS = (0, 2, 4)


@functools.lru_cache(maxsize=None)
def reads():
    """(name, read): the shared reads, then windows of 100 bases with substitutions at the given positions -- the longest exact stretch is the seed, what lies
    right of it is the right clip --, windows whose right flank holds a variant site, every second one reverse-complemented"""
    S, o = XC.toy()
    rng = np.random.default_rng(202)
    unit = S.L + S.pad
    out = [q for _, q in XC.reads(S)]
    plans = [(60,), (30, 70), (20, 25, 80), (60, 90, 92, 94, 96), (70, 85), (10, 55), (45, 47, 49, 51, 53, 95), (64, 99)]
    for i in range(32):
        h, s = i % S.H, int(rng.integers(40, S.L - 140))
        q = bytearray(S.text[h * unit + s:h * unit + s + 100].tobytes())
        for p in plans[i % len(plans)]:
            XC._sub(q, p)
        if i % 16 == 9:
            q[88] = ord("N")
        out.append(bytes(q))
    for si, site in enumerate(S.sites):                      # a variant site 15 bases right of a planted substitution, the seed left of both
        site = int(site)
        if 70 <= site < S.L - 40:
            q = bytearray(S.text[(si % S.H) * unit + site - 60:(si % S.H) * unit + site + 30].tobytes())
            XC._sub(q, 45)
            out.append(bytes(q))
    for h in range(S.H):                                     # a window that ends with its document (the separator included), then foreign bases: the limit cuts the walk
        q = bytearray(S.text[h * unit + S.L - 50:(h + 1) * unit].tobytes()) + bytearray(b"ACGTTGCAAC")
        XC._sub(q, 35)
        out.append(bytes(q))
    out = [SAM.revcomp(q) if i % 2 else q for i, q in enumerate(out)]
    return tuple((b"y%d" % i, q) for i, q in enumerate(out))


@functools.lru_cache(maxsize=None)
def model():
    S, o = XC.toy()
    return FM.FL(S.heads, S.lens)


@functools.lru_cache(maxsize=None)
def records(K):
    S, o = XC.toy()
    return [FM.read_records_both(o, model(), S.doc_starts, q, XC.MIN_LENGTH, XC.MAX_HITS, True, K) for _, q in reads()]


def kinds(K):
    seen = set()
    for (_, q), recs in zip(reads(), records(K)):
        if recs == [None]:
            continue
        mds = set()
        for (lo, hi, k, a, b, rev), j, l, dn, offs, x, y in recs:
            m = len(q)
            if m > b and y["ext"] == m - b:
                seen.add("right clip gone")
            if m > b and 0 < y["ext"] < m - b:
                seen.add("right clip shortened")
            if x["ext"] > 0 and y["ext"] > 0:
                seen.add("both clips moved")
            if x["nm"] > 0 and y["nm"] > 0 and x["nm"] + y["nm"] == K:
                seen.add("budget split")
            if m > b and y is not FM.ZERO and x["nm"] == K and K > 0:
                seen.add("budget exhausted by the left walk")
            if rev and y["ext"] > 0:
                seen.add("reverse")
            if a == 0 and b == m:
                seen.add("exact")
            if y["why"] == "length" and y["steps"] < m - b:
                seen.add("cut by the document's end")
            mds.add(tuple(y["mis"][:y["nm"]]))
        if len(recs) >= 2 and len(mds) >= 2:
            seen.add("secondary lines of different right MD")
    return seen


def test_inputs_hold_every_kind_of_line():
    assert kinds(4) >= {"right clip gone", "right clip shortened", "both clips moved", "reverse", "exact", "secondary lines of different right MD",
                        "cut by the document's end"}, kinds(4)
    assert {"budget split", "budget exhausted by the left walk"} <= kinds(2), kinds(2)
    S, o = XC.toy()
    for K in KS:                                             # NM never exceeds the budget; the seed and both flanks re-expand to the text
        for (_, q), recs in zip(reads(), records(K)):
            if recs == [None]:
                continue
            for (lo, hi, k, a, b, rev), j, l, dn, offs, x, y in recs:
                s = SAM.revcomp(q) if rev else q
                assert x["nm"] + y["nm"] <= K
                er = y["ext"]
                ref, mine = S.text[l + b - a:l + b - a + er].tobytes(), s[b:b + er]
                assert [(t, ref[t]) for t in range(er) if ref[t] != mine[t]] == y["mis"][:y["nm"]]
                assert er == 0 or ref[er - 1] == mine[er - 1]


@pytest.fixture(scope="module", params=[(capi.LAYOUT_SLOTS, 0), (capi.LAYOUT_RUNS, 0), (capi.LAYOUT_SLOTS, 8), (capi.LAYOUT_RUNS, 8)],
                ids=["slots", "runs", "slots-8-byte", "runs-8-byte"])
def toy(request):
    S, o = XC.toy()
    layout, pos_bytes = request.param
    with capi.default_option(capi.OPT_POS_BYTES, pos_bytes):
        rb = _with_layout(layout, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    assert rb.info().pos_bytes == (pos_bytes or 4)
    rb.set_docs(S.doc_names, S.doc_starts)
    yield S, rb, o
    rb.close()


def _same(got, want):
    if got == want:
        return
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    m = min(len(a), len(b))
    d = np.nonzero(a[:m] != b[:m])[0]
    at = int(d[0]) if len(d) else m
    raise AssertionError(f"texts differ at byte {at} (got {len(got)} bytes, want {len(want)}): got {got[max(at - 80, 0):at + 80]!r}, "
                         f"want {want[max(at - 80, 0):at + 80]!r}")


def test_not_loaded_then_the_whole_text(toy, monkeypatch):
    S, rb, o = toy
    rs = reads()
    names, seqs, quals = [n for n, _ in rs], [q for _, q in rs], XC.quals(rs)
    if not rb.fl_info()["prepared"]:
        with pytest.raises(ra.RbgError) as ei:
            rb.align_sam_extend(seqs, None, names, right=True)
        assert ei.value.code == ENOTLOADED
        rb.fl_prepare()
    for K in KS:
        for secondary in (False, True):
            ql = quals if K == 4 else None
            want = FM.lines_both(o, model(), S.doc_starts, names, seqs, ql, XC.MIN_LENGTH, XC.MAX_HITS, secondary, K)
            before = rb.counters().astype(np.int64)
            got = rb.align_sam_extend(seqs, ql, names, XC.MIN_LENGTH, XC.MAX_HITS, secondary, K, right=True)
            mid = rb.counters().astype(np.int64)
            _same(got, b"".join(want))
            left = rb.align_sam_extend(seqs, ql, names, XC.MIN_LENGTH, XC.MAX_HITS, secondary, K)
            after = rb.counters().astype(np.int64)
            assert (after - mid == mid - before).all() and int((mid - before)[0]) == 2 * len(seqs)          # counters as the left call
            # lines without a right clip are the left call's lines
            gl, ll = got.splitlines(keepends=True), left.splitlines(keepends=True)
            assert len(gl) == len(ll)
            noclip = [i for i, l in enumerate(ll) if l.split(b"\t")[1] != b"4" and not l.split(b"\t")[5].endswith(b"S")]
            assert len(noclip) >= 10 and all(gl[i] == ll[i] for i in noclip)
            assert K == 0 or any(g != l for g, l in zip(gl, ll))
    monkeypatch.setenv("RBG_SAM_GRID_CAP", "1")              # one workgroup strides through every kernel
    want = FM.lines_both(o, model(), S.doc_starts, names, seqs, None, 20, 16, True, 4)
    _same(rb.align_sam_extend(seqs * 5, None, names * 5, 20, 16, True, 4, right=True), b"".join(want) * 5)
    monkeypatch.delenv("RBG_SAM_GRID_CAP")


def test_lines_at_the_staging_limit(toy):
    """a workgroup's lines of exactly kSamLds bytes (staged) and of kSamLds + 1 (every lane writes its own line), lines with right mismatches in MD among them"""
    S, rb, o = toy
    rb.fl_prepare()
    limit, per = 48 * 1024, 128
    with open(capi.__file__.replace("capi.py", "csrc/fl_extend.hip")) as f:
        src = f.read()
    assert re.search(r"kSamLds\s*=\s*48\s*\*\s*1024\s*;", src) and re.search(r"kSamLines\s*=\s*128\s*;", src)
    rng = np.random.default_rng(10)
    pool = [q for _, q in reads() if len(q) >= 60]
    pool_q = XC.quals([(b"", q) for q in pool])
    tails = [FM.read_lines_both(o, model(), S.doc_starts, b"", q, ql, XC.MIN_LENGTH, 1, False, 4) for q, ql in zip(pool, pool_q)]
    assert all(len(t) == 1 for t in tails)
    tails = [t[0] for t in tails]

    def run(targets):
        n = per * len(targets)
        idx = [(i * 7 + i // per) % len(pool) for i in range(n)]
        names = []
        for b, t in enumerate(targets):
            blk = [len(tails[j]) for j in idx[per * b:per * (b + 1)]]
            need = t - sum(blk)
            assert need >= 0, (b, t, sum(blk))
            q, r = divmod(need, len(blk))
            names += [bytes(rng.integers(ord("a"), ord("z") + 1, q + (1 if j < r else 0), dtype=np.uint8)) for j in range(len(blk))]
        want = [nm + tails[j] for nm, j in zip(names, idx)]
        _same(rb.align_sam_extend([pool[j] for j in idx], [pool_q[j] for j in idx], names, XC.MIN_LENGTH, 1, False, 4, right=True), b"".join(want))
        return [sum(len(e) for e in want[b:b + per]) for b in range(0, n, per)]

    assert run([47000, limit, limit + 1, 47000]) == [47000, limit, limit + 1, 47000]


def test_a_prepared_replica(toy):
    S, rb, o = toy
    rb.fl_prepare()
    rs = reads()
    names, seqs = [n for n, _ in rs], [q for _, q in rs]
    rep = rb.replicate(0)
    try:
        with pytest.raises(ra.RbgError) as ei:
            rep.align_sam_extend(seqs, None, names, right=True)
        assert ei.value.code == ENOTLOADED
        rep.fl_prepare()
        _same(rep.align_sam_extend(seqs, None, names, 20, 8, True, 4, right=True),
              b"".join(FM.lines_both(o, model(), S.doc_starts, names, seqs, None, 20, 8, True, 4)))
    finally:
        rep.close()
    assert rb.align_sam_extend([], None, [], right=True) == b""
