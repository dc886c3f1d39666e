"""GPU parity of rbg_align_sam / rbg_sam_header (k_sam.hip, capi/sam.ipp) against tests/sam_model.py: every comparison is of the whole output, byte for
byte.  A case built to reach a branch of k_sam_write asserts from the EXPECTED text that it does: the bytes of lines kSamLines b .. kSamLines b + kSamLines - 1
are summed and compared with kSamLds, both read from the kernel's source."""
import os
import re

import numpy as np
import pytest

import orc
import rowbowt_amd as ra
import sam_model as SAM
from rowbowt_amd import capi
from gpu_common import _with_layout
from synth import SynthIndex

pytestmark = pytest.mark.gpu
M64 = 2**64 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EARG, ENOTLOADED = -4, -6


def _const(name, pattern=r"(\d+)"):
    with open(os.path.join(ROOT, "rowbowt_amd", "csrc", "k_sam.hip")) as f:
        m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*%s\s*;" % (name, pattern), f.read())
    assert m, f"{name} not found in k_sam.hip: this file's boundary cases follow that constant"
    return m


def _limits():
    return int(_const("kSamLds", r"(\d+)\s*\*\s*1024").group(1)) * 1024, int(_const("kSamLines").group(1))


def _same(got, want):
    if got == want:
        return
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    m = min(len(a), len(b))
    d = np.nonzero(a[:m] != b[:m])[0]
    at = int(d[0]) if len(d) else m
    raise AssertionError(f"texts differ at byte {at} (got {len(got)} bytes, want {len(want)}): got {got[max(at - 80, 0):at + 80]!r}, "
                         f"want {want[max(at - 80, 0):at + 80]!r}")


def _block_bytes(lines, per):
    return [sum(len(e) for e in lines[b:b + per]) for b in range(0, len(lines), per)]


def _letters(rng, n):
    return bytes(rng.integers(ord("a"), ord("z") + 1, n, dtype=np.uint8))


def _quals(reads, salt=0):
    return [bytes(33 + (j * 5 + i + salt) % 60 for j in range(len(q))) for i, q in enumerate(reads)]


TOY = dict(L=1500, H=5, n_sites=30, seed=23)


@pytest.fixture(scope="module")
def toy_index():
    S = SynthIndex(**TOY)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    o.set_docs(S.doc_names, S.doc_starts)
    yield S, o
    o.close()


@pytest.fixture(scope="module", params=[capi.LAYOUT_SLOTS, capi.LAYOUT_RUNS], ids=["slots", "runs"])
def toy(request, toy_index):
    S, o = toy_index
    rb = _with_layout(request.param, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    rb.set_docs(S.doc_names, S.doc_starts)
    yield S, rb, o
    rb.close()


def _toy_reads(S):
    """every shape of read: lengths 0 .. 150 around the 16-byte pieces, whole matches on each strand, one and two substitutions, N, lower case, no match on
    either strand, a read that is its own reverse complement (the tie)"""
    rng = np.random.default_rng(77)
    unit = S.L + S.pad
    reads = []
    for i, m in enumerate((0, 1, 15, 16, 17, 63, 64, 65, 150) * 2):
        s = (i % S.H) * unit + int(rng.integers(0, S.L - 150))
        q = S.text[s:s + m].tobytes()
        reads.append(SAM.revcomp(q) if i >= 9 else q)
    base = S.sample_reads(24, 80, seed=8, sub_rate=0.0, ragged=True)
    for i, q in enumerate(base):
        q = bytearray(q)
        if i % 4 in (1, 2) and len(q) > 8:                      # one or two substitutions
            for p in rng.choice(len(q), i % 4, replace=False):
                q[p] = ord("ACGT"[("ACGT".index(chr(q[p])) + 1) % 4])
        if i % 6 == 5 and len(q) > 4:
            q[len(q) // 3] = ord("N")
        q = bytes(q)
        reads.append(SAM.revcomp(q) if i % 2 else q)
    half = S.text[300:320].tobytes()
    reads += [half + b"N" + SAM.revcomp(half), S.text[700:760].tobytes().lower(), S.text[700:730].tobytes() + S.text[730:760].tobytes().lower(),
              b"N" * 40, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 70)), b"ACGTN" * 5, S.text[40:52].tobytes(), SAM.revcomp(S.text[40:59].tobytes())]
    return reads


def test_every_shape_of_read(toy):
    S, rb, o = toy
    reads = _toy_reads(S)
    names = [b"read%d" % i if i % 5 else b"" for i in range(len(reads))]
    quals = _quals(reads)
    kinds = set()
    for min_length in (1, 10, 20):
        for max_hits, secondary in ((1, False), (3, False), (16, False), (M64, False), (1, True), (3, True), (M64, True), (0, True)):
            for ql in (quals, None):
                want = SAM.lines(o, names, reads, ql, min_length, max_hits, secondary)
                _same(rb.align_sam(reads, ql, names, min_length, max_hits, secondary), b"".join(want))
                kinds |= {int(l.split(b"\t")[1]) for l in want}
                if min_length == 20:
                    assert sum(1 for l in want if l.split(b"\t")[1] == b"4") >= 8      # no match, or shorter than min_length
    assert kinds == {0, 4, 16, 256, 272}
    pal = S.text[300:320].tobytes() + b"N" + SAM.revcomp(S.text[300:320].tobytes())   # its own reverse complement: both strands hold the same seed
    assert pal in reads and SAM.revcomp(pal) == pal and SAM.pick(o, pal, 10)[3:] == (0, 20, 0)                 # the tie goes to forward


def _padded_names(base, targets, per, rng):
    names = []
    for b, t in enumerate(targets):
        blk = base[per * b:per * (b + 1)]
        need = t - sum(blk)
        assert blk and need >= 0, (b, t, sum(blk))
        q, r = divmod(need, len(blk))
        names += [_letters(rng, q + (1 if j < r else 0)) for j in range(len(blk))]
    assert len(names) == len(base)
    return names


def test_lines_at_the_staging_limit(toy_index):
    """k_sam_write's two paths and the copy-out of the staged one: a workgroup's lines of exactly kSamLds bytes (staged), the next of kSamLds + 1 (every lane
    writes its line to memory), a short one -- behind a leading block of s more than a multiple of 16 bytes for s = 0 .. 15, the alignment of the staged
    block's first byte; a last block that is partial and over the limit"""
    S, o = toy_index
    rb = ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0)
    rb.set_docs(S.doc_names, S.doc_starts)
    limit, per = _limits()
    rng = np.random.default_rng(6)
    pool = S.sample_reads(40, 60, seed=12, sub_rate=0.3, ragged=True)
    pool = [SAM.revcomp(q) if i % 2 else q for i, q in enumerate(pool)] + [b"", b"NNNN"]
    pool_q = _quals(pool)
    tails = [SAM.read_lines(o, b"", q, ql, 15, 1, False) for q, ql in zip(pool, pool_q)]      # the model's line of every pool read, its name empty
    assert all(len(t) == 1 for t in tails)
    tails = [t[0] for t in tails]
    assert {int(t.split(b"\t")[1]) for t in tails} == {0, 4, 16}

    def run(n, targets):
        idx = [(i * 7 + i // per) % len(pool) for i in range(n)]
        reads, quals = [pool[j] for j in idx], [pool_q[j] for j in idx]
        names = _padded_names([len(tails[j]) for j in idx], targets, per, rng)
        want = [nm + tails[j] for nm, j in zip(names, idx)]                                     # (a name is the line's first bytes and nothing else)
        _same(rb.align_sam(reads, quals, names, 15, 1, False), b"".join(want))
        return _block_bytes(want, per)

    shifts = set()
    for s in range(16):
        lead = 20000 + (s - 20000) % 16
        got = run(4 * per, [lead, limit, limit + 1, 18000])
        assert got == [lead, limit, limit + 1, 18000] and lead % 16 == s
        shifts.add(got[0] % 16)
    assert shifts == set(range(16))
    assert run(per + per // 3, [18000, limit + 77]) == [18000, limit + 77]       # E no multiple of kSamLines, the partial block unstaged
    rb.close()


def test_one_line_longer_than_the_limit(toy_index):
    """a name of 70 000 bytes and a read of 40 000 bp (mapped on the reverse strand by a seed inside it, and unmapped): their blocks go straight to memory,
    the blocks around them are staged"""
    S, o = toy_index
    rb = ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0)
    rb.set_docs(S.doc_names, S.doc_starts)
    limit, per = _limits()
    rng = np.random.default_rng(16)
    reads = S.sample_reads(3 * per + 10, 40, seed=2, sub_rate=0.2)
    names = [b"n%d" % i for i in range(len(reads))]
    names[per + 5] = _letters(rng, 70000)
    junk = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 40000))
    long_read = bytearray(junk)
    long_read[20000:20060] = S.text[200:260].tobytes()
    reads[2 * per + 9] = SAM.revcomp(bytes(long_read))
    assert SAM.pick(o, reads[2 * per + 9], 20)[5] == 1
    quals = _quals(reads)
    want = SAM.lines(o, names, reads, quals, 20, 1, False)
    sums = _block_bytes(want, per)
    assert len(sums) == 4 and sums[0] <= limit and sums[1] > limit and sums[2] > limit and sums[3] <= limit
    assert want[2 * per + 9].split(b"\t")[1] == b"16" and len(want[2 * per + 9]) > 80000
    _same(rb.align_sam(reads, quals, names, 20, 1, False), b"".join(want))
    reads[2 * per + 9] = junk.replace(b"A", b"N")                                # unmapped, 40 000 bytes as given, no qualities
    one = SAM.read_lines(o, names[2 * per + 9], reads[2 * per + 9], None, 20, 1, False)
    want = [l.rsplit(b"\t", 3 if l.split(b"\t")[1] != b"4" else 1) for l in want]             # the same lines with QUAL "*"
    want = [b"\t".join([x[0], b"*"] + x[2:]) if len(x) == 4 else x[0] + b"\t*\n" for x in want]
    want[2 * per + 9] = one[0]
    assert one[0].split(b"\t")[1] == b"4" and len(one[0]) > 40000
    _same(rb.align_sam(reads, None, names, 20, 1, False), b"".join(want))
    rb.close()


def test_grid_stride_turns(toy, monkeypatch):
    """RBG_SAM_GRID_CAP=2: every kernel of k_sam.hip goes round its grid-stride loop many times -- 3 000 reads with secondaries, neither the reads nor the
    lines a multiple of the block sizes"""
    S, rb, o = toy
    _, per = _limits()
    reads = S.sample_reads(3001, 30, seed=21, sub_rate=0.2, ragged=True)
    reads = [SAM.revcomp(q) if i % 3 == 1 else q for i, q in enumerate(reads)]
    names = [b"g%d" % i for i in range(len(reads))]
    quals = _quals(reads, 3)
    want = SAM.lines(o, names, reads, quals, 12, 4, True)
    assert len(reads) % 256 and len(want) % per and len(want) % 256 and len(want) > len(reads) + 500 and len(want) > 2 * 2 * 256
    monkeypatch.setenv("RBG_SAM_GRID_CAP", "2")
    _same(rb.align_sam(reads, quals, names, 12, 4, True), b"".join(want))
    monkeypatch.delenv("RBG_SAM_GRID_CAP")
    _same(rb.align_sam(reads, quals, names, 12, 4, True), b"".join(want))


def test_ordered_walk_and_counters(toy):
    """a batch large enough for the locate order (4 096 reads and more); rbg_counters: 2 N reads searched, every location walked once"""
    S, rb, o = toy
    reads = S.sample_reads(4200, 24, seed=33, sub_rate=0.1)
    reads = [SAM.revcomp(q) if i % 2 else q for i, q in enumerate(reads)]
    names = [b"c%d" % i for i in range(len(reads))]
    want = SAM.lines(o, names, reads, None, 16, 5, True)
    before = rb.counters().astype(np.int64)
    _same(rb.align_sam(reads, None, names, 16, 5, True), b"".join(want))
    delta = rb.counters().astype(np.int64) - before
    nlocs = sum(1 for l in want if l.split(b"\t")[1] != b"4")
    assert nlocs > len(reads) and int(delta[0]) == 2 * len(reads) and int(delta[3]) == nlocs


def test_decimals(synth):
    """POS of 1 to 5 digits (one document over the whole text of n = 32 081) and NH:i: / HI:i: of 1 to 4 digits (short reads of a text with long repeats, every
    location listed); the powers of ten themselves where the index has them"""
    S = synth
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    rb = _with_layout(capi.LAYOUT_RUNS, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    rb.set_docs(["only"], [0])
    o.set_docs(["only"], [0])
    text = S.text.tobytes()
    reads = [text[p:p + 25] for p in (0, 8, 9, 10, 98, 99, 100, 998, 999, 1000, 9998, 9999, 10000, 31000)]   # POS = p + 1 for a unique read
    reads += [b"A" * 10, b"A" * 9, b"A" * 3, b"AC", b"ACG", b"ACGT", b"T", b"GGA", b"CATG"]
    names = [b"d%d" % i for i in range(len(reads))]
    want = SAM.lines(o, names, reads, None, 1, M64, True)
    f = [l[:-1].split(b"\t") for l in want]
    pos = {int(x[3]) for x in f}
    assert {len(str(p)) for p in pos} == {1, 2, 3, 4, 5} and {1, 9, 10, 99, 100, 999, 1000, 9999, 10000} <= pos
    assert {len(x[11]) - 5 for x in f} == {1, 2, 3, 4} and {len(x[12]) - 5 for x in f} == {1, 2, 3, 4}
    his = {int(x[12][5:]) for x in f}
    assert {9, 10, 99, 100, 999, 1000} <= his
    _same(rb.align_sam(reads, None, names, 1, M64, True), b"".join(want))
    rb.close()
    o.close()


def test_document_table_at_its_edges(toy_index):
    """locations equal to a document's start and to a start - 1; names of 0, 1 and 300 bytes; starts given out of order; a first document that starts behind a
    location (RBG_EARG, and the next call with a valid table is right); the header of each table"""
    S, o = toy_index
    rb = ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0)
    reads = S.sample_reads(300, 30, seed=5, sub_rate=0.1)
    reads = [SAM.revcomp(q) if i % 2 else q for i, q in enumerate(reads)]
    names = [b"e%d" % i for i in range(len(reads))]
    picks = [SAM.pick(o, q, 12) for q in reads]
    U = sorted({l for p in picks if p for l in o.locs_at(p[0], p[1], p[2], 6)})
    q = len(U) // 5
    starts = sorted({0, U[q], U[2 * q] + 1, U[3 * q], U[3 * q] + 1, U[4 * q]})
    dnames = ["", "a", "x" * 300] + [f"doc{j}" for j in range(3, len(starts))]
    try:
        for dn, st in ((dnames, starts), (dnames, starts[::-1]), (dnames, starts[2:] + starts[:2]), (["only"], [0])):
            rb.set_docs(dn, st)
            o.set_docs(dn, st)
            want = SAM.lines(o, names, reads, None, 12, 6, True)
            assert want is not None
            _same(rb.align_sam(reads, None, names, 12, 6, True), b"".join(want))
            _same(rb.sam_header(), SAM.header(dn, st, S.n))
        bad = [U[0] + 1, U[len(U) // 2]]
        rb.set_docs(["late", "z"], bad)
        o.set_docs(["late", "z"], bad)
        assert SAM.lines(o, names, reads, None, 12, 6, True) is None
        with pytest.raises(ra.RbgError) as ei:
            rb.align_sam(reads, None, names, 12, 6, True)
        assert ei.value.code == EARG
        rb.set_docs(dnames, starts)
        o.set_docs(dnames, starts)
        _same(rb.align_sam(reads, None, names, 12, 6, True), b"".join(SAM.lines(o, names, reads, None, 12, 6, True)))
    finally:
        o.set_docs(S.doc_names, S.doc_starts)
        rb.close()


def test_header(toy):
    S, rb, o = toy
    _same(rb.sam_header(), SAM.header(S.doc_names, S.doc_starts, S.n))
    pg = b"@PG\tID:rb_align\tPN:rb_align\n@CO\tno newline at the end"
    _same(rb.sam_header(pg), SAM.header(S.doc_names, S.doc_starts, S.n, pg))
    assert rb.info().n == S.n


def test_errors_and_edge_batches(toy_index):
    S, o = toy_index
    reads, names = [S.text[100:140].tobytes()], [b"x"]
    rb = ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0)
    with pytest.raises(ra.RbgError) as ei:                                      # no documents
        rb.align_sam(reads, None, names)
    assert ei.value.code == ENOTLOADED
    with pytest.raises(ra.RbgError) as ei:
        rb.sam_header()
    assert ei.value.code == ENOTLOADED
    rb.set_docs(S.doc_names, S.doc_starts)
    with pytest.raises(ra.RbgError) as ei:
        rb.align_sam(reads, None, names, min_length=0)
    assert ei.value.code == EARG
    L = rb.L
    text, n = capi.VP(), capi.U64()
    import ctypes as C
    args = lambda N, flags: (rb.h, b"ACGT", capi._p(np.zeros(1, np.uint64)), capi._p(np.full(1, 4, np.uint32)), None, None, b"x", capi._p(np.zeros(1, np.uint64)),
                             capi._p(np.ones(1, np.uint32)), N, 20, 16, flags, C.byref(text), C.byref(n))
    assert L.rbg_align_sam(*args(1, 2)) == EARG and L.rbg_align_sam(*args(1, 0x80000001)) == EARG      # unknown flags
    assert L.rbg_align_sam(*args(1 << 32, 0)) == EARG
    # 2^32 or more bytes of reads, or of names: answered from the lengths alone (two spans of 2^31 bytes; no byte of them is read)
    big, one, beg = np.full(2, 1 << 31, np.uint32), np.ones(2, np.uint32), np.zeros(2, np.uint64)
    for sl, nl in ((big, one), (one, big)):
        assert L.rbg_align_sam(rb.h, b"AC", capi._p(beg), capi._p(sl), None, None, b"xy", capi._p(beg), capi._p(nl), 2, 20, 16, 0, C.byref(text), C.byref(n)) == EARG
    text.value, n.value = 1, 7
    assert L.rbg_align_sam(*args(0, 0)) == 0 and text.value is None and n.value == 0                   # N == 0
    assert rb.align_sam([], None, []) == b""
    _same(rb.align_sam(reads, None, names), SAM.text(o, names, reads, None))                           # N == 1
    _same(rb.align_sam([b""], [b""], [b"empty"]), b"empty\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n")
    rb.close()
    nosa = ra.RowBowt.from_runs(S.heads, S.lens, device=0)                      # no toehold SA
    nosa.set_docs(S.doc_names, S.doc_starts)
    with pytest.raises(ra.RbgError) as ei:
        nosa.align_sam(reads, None, names)
    assert ei.value.code == ENOTLOADED
    nosa.close()


def test_replica_and_two_buffers_out(toy):
    """a replica gives its primary's bytes; two texts of one handle are out at once, each intact after the other was made, then released"""
    import ctypes as C
    S, rb, o = toy
    reads = S.sample_reads(500, 40, seed=9, sub_rate=0.2)
    reads = [SAM.revcomp(q) if i % 2 else q for i, q in enumerate(reads)]
    names = [b"b%d" % i for i in range(len(reads))]
    quals = _quals(reads)
    want = SAM.text(o, names, reads, quals, 20, 4, True)
    rep = rb.replicate(0)
    try:
        _same(rep.align_sam(reads, quals, names, 20, 4, True), want)
        _same(rep.sam_header(), rb.sam_header())
    finally:
        rep.close()
    half = len(reads) // 2

    def raw(lo, hi):
        sub = reads[lo:hi]
        sl = np.array([len(x) for x in sub], np.uint32)
        sb = np.concatenate(([0], np.cumsum(sl[:-1]))).astype(np.uint64)
        nl = np.array([len(x) for x in names[lo:hi]], np.uint32)
        nb = np.concatenate(([0], np.cumsum(nl[:-1]))).astype(np.uint64)
        text, n = capi.VP(), capi.U64()
        rc = rb.L.rbg_align_sam(rb.h, b"".join(sub), capi._p(sb), capi._p(sl), b"".join(quals[lo:hi]), capi._p(sb), b"".join(names[lo:hi]), capi._p(nb),
                                capi._p(nl), hi - lo, 20, 4, capi.SAM_SECONDARY, C.byref(text), C.byref(n))
        assert rc == 0
        return text, n.value

    t1, n1 = raw(0, half)
    t2, n2 = raw(half, len(reads))
    assert t1.value != t2.value
    assert rb.L.rbg_wait_text(rb.h, t1) == 0 and rb.L.rbg_wait_text(rb.h, t2) == 0
    got = C.string_at(t1, n1) + C.string_at(t2, n2)
    assert rb.L.rbg_release_text(rb.h, t1) == 0 and rb.L.rbg_release_text(rb.h, t2) == 0
    _same(got, want)
