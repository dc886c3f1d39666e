"""GPU parity of rbg_align_sam_extend (sam_extend.hip, capi/sam.ipp) against tests/sam_extend_model.py on the shared inputs of tests/sam_extend_cases.py
(tests/test_sam_extend_model.py asserts on the CPU which kinds of line they hold): every comparison is of the whole output, byte for byte."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rowbowt_amd as ra
import sam_extend_cases as XC
import sam_extend_model as XM
import sam_model as SAM
from rowbowt_amd import capi
from gpu_common import _with_layout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EARG = -4


def _limits():
    with open(os.path.join(ROOT, "rowbowt_amd", "csrc", "sam_extend.hip")) as f:
        src = f.read()
    lds = re.search(r"constexpr\s+uint32_t\s+kSamLds\s*=\s*(\d+)\s*\*\s*1024\s*;", src)
    per = re.search(r"constexpr\s+uint32_t\s+kSamLines\s*=\s*(\d+)\s*;", src)
    assert lds and per, "kSamLds / kSamLines not found in sam_extend.hip: the staging cases follow those constants"
    return int(lds.group(1)) * 1024, int(per.group(1))


def _same(got, want):
    if got == want:
        return
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    m = min(len(a), len(b))
    d = np.nonzero(a[:m] != b[:m])[0]
    at = int(d[0]) if len(d) else m
    raise AssertionError(f"texts differ at byte {at} (got {len(got)} bytes, want {len(want)}): got {got[max(at - 80, 0):at + 80]!r}, "
                         f"want {want[max(at - 80, 0):at + 80]!r}")


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


@pytest.mark.parametrize("K", (0, 4))
@pytest.mark.parametrize("secondary", (False, True))
def test_shared_reads(toy, K, secondary):
    S, rb, o = toy
    rs = XC.reads(S)
    names, reads, quals = [n for n, _ in rs], [q for _, q in rs], XC.quals(rs)
    for ql in (quals, None):
        want = XM.lines(o, names, reads, ql, XC.MIN_LENGTH, XC.MAX_HITS, secondary, K)
        _same(rb.align_sam_extend(reads, ql, names, XC.MIN_LENGTH, XC.MAX_HITS, secondary, K), b"".join(want))
    if K == 4:
        tags = [l[:-1].split(b"\t")[13:] for l in want if l.split(b"\t")[1] != b"4"]
        assert all(len(t) == 3 for t in tags) and any(t[0] != b"NM:i:0" for t in tags) and any(re.search(rb"[ACGT]", t[1][5:]) for t in tags)


def test_default_budget_and_one_workgroup(toy, monkeypatch):
    S, rb, o = toy
    rs = XC.reads(S)
    names, reads = [n for n, _ in rs], [q for _, q in rs]
    want = XM.text(o, names, reads, None, 20, 16, True, 4)
    _same(rb.align_sam_extend(reads, None, names, secondary=True), want)                     # max_mismatch = 4 by default
    monkeypatch.setenv("RBG_SAM_GRID_CAP", "1")
    _same(rb.align_sam_extend(reads * 7, None, names * 7, 20, 16, True, 4), want * 7)         # 385 reads, more than a thousand lines: every kernel strides
    monkeypatch.delenv("RBG_SAM_GRID_CAP")


def test_lines_at_the_staging_limit(toy):
    """a workgroup's lines of exactly kSamLds bytes (staged) and of kSamLds + 1 (every lane writes its own line), lines with mismatches in MD among them --
    the lengths come from k_sam_len_ext, a byte too few or too many in sam_md_len moves every later line"""
    S, rb, o = toy
    limit, per = _limits()
    rng = np.random.default_rng(9)
    pool = [q for _, q in XC.reads(S)]
    pool_q = XC.quals(XC.reads(S))
    tails = [XM.read_lines(o, b"", q, ql, XC.MIN_LENGTH, 1, False, 4) for q, ql in zip(pool, pool_q)]
    assert all(len(t) == 1 for t in tails)
    tails = [t[0] for t in tails]
    assert sum(1 for t in tails if re.search(rb"MD:Z:\d+[ACGT]", t)) >= 10

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
        assert any(re.search(rb"MD:Z:\d+[ACGT]", w) for w in want[per:3 * per])
        _same(rb.align_sam_extend([pool[j] for j in idx], [pool_q[j] for j in idx], names, XC.MIN_LENGTH, 1, False, 4), b"".join(want))
        return [sum(len(e) for e in want[b:b + per]) for b in range(0, n, per)]

    for s in (0, 5, 15):
        lead = 40000 + (s - 40000) % 16
        assert run([lead, limit, limit + 1, 38000]) == [lead, limit, limit + 1, 38000] and lead % 16 == s


def test_exact_reads_get_the_three_tags_only(toy):
    """every read maps with a = 0: the extended output is rbg_align_sam's with NM:i:0 MD:Z:<b - a> AS:i:<b - a> appended to the mapped lines; and the
    counters move as rbg_align_sam's do"""
    S, rb, o = toy
    reads = [S.text[(i % S.H) * (S.L + S.pad) + 13 * i:(i % S.H) * (S.L + S.pad) + 13 * i + 50 + i % 30].tobytes() for i in range(90)]
    reads = [SAM.revcomp(q) if i % 2 else q for i, q in enumerate(reads)] + [b"N" * 25]
    names = [b"r%d" % i for i in range(len(reads))]
    assert all(p is None or p[3] == 0 for p in (SAM.pick(o, q, 20) for q in reads))
    before = rb.counters().astype(np.int64)
    plain = rb.align_sam(reads, None, names, 20, 4, True)
    mid = rb.counters().astype(np.int64)
    ext = rb.align_sam_extend(reads, None, names, 20, 4, True, 4)
    after = rb.counters().astype(np.int64)
    want = []
    for l in plain.splitlines(keepends=True):
        f = l[:-1].split(b"\t")
        if f[1] != b"4":
            m = int(re.fullmatch(rb"(\d+)M(?:\d+S)?", f[5]).group(1))
            l = l[:-1] + b"\tNM:i:0\tMD:Z:%d\tAS:i:%d\n" % (m, m)
        want.append(l)
    assert len(want) > len(reads) and want[-1].split(b"\t")[1] == b"4"
    _same(ext, b"".join(want))
    assert (after - mid == mid - before).all() and int((mid - before)[0]) == 2 * len(reads) and int((mid - before)[3]) == len(want) - 1


def test_errors_and_edge_batches(toy):
    S, rb, o = toy
    reads, names = [S.text[100:140].tobytes()], [b"x"]
    with pytest.raises(ra.RbgError) as ei:
        rb.align_sam_extend(reads, None, names, max_mismatch=9)
    assert ei.value.code == EARG
    with pytest.raises(ra.RbgError) as ei:
        rb.align_sam_extend(reads, None, names, min_length=0)
    assert ei.value.code == EARG
    assert rb.align_sam_extend([], None, []) == b""                                            # N == 0
    text, n = capi.VP(1), capi.U64(7)
    assert rb.L.rbg_align_sam_extend(rb.h, None, None, None, None, None, None, None, None, 0, 20, 16, 0, 4, C.byref(text), C.byref(n)) == 0
    assert text.value is None and n.value == 0
    assert rb.L.rbg_align_sam_extend(rb.h, None, None, None, None, None, None, None, None, 0, 20, 16, 2, 4, C.byref(text), C.byref(n)) == EARG   # unknown flags
    _same(rb.align_sam_extend(reads, None, names), XM.text(o, names, reads, None))            # N == 1
    rep = rb.replicate(0)
    try:
        rs = XC.reads(S)
        _same(rep.align_sam_extend([q for _, q in rs], None, [n_ for n_, _ in rs], 20, 8, True, 4), XM.text(o, [n_ for n_, _ in rs], [q for _, q in rs], None, 20, 8, True, 4))
    finally:
        rep.close()
