"""The SAM model (tests/sam_model.py: what rbg_align_sam and rbg_sam_header must produce) against the text itself on a synthetic pangenome with several
documents, and the binding surface of the two calls.  No GPU."""
import re

import numpy as np
import pytest

import orc
import sam_model as SAM
from synth import SynthIndex


@pytest.fixture(scope="module")
def case():
    S = SynthIndex(L=1200, H=4, n_sites=25, seed=31)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    o.set_docs(S.doc_names, S.doc_starts)
    yield S, o
    o.close()


def _reads(S):
    fwd = S.sample_reads(60, 50, seed=3, sub_rate=0.5, ragged=True)
    rng = np.random.default_rng(4)
    reads = []
    for i, q in enumerate(fwd):
        q = SAM.revcomp(q) if i % 2 else q
        if i % 7 == 3 and len(q) > 12:
            q = q[:len(q) // 2] + b"N" + q[len(q) // 2 + 1:]
        reads.append(q)
    reads += [b"", b"A", b"N" * 30, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 40)), S.text[100:140].tobytes().lower()]
    return reads


def _parse_cigar(c):
    return [(int(n), op) for n, op in re.findall(rb"(\d+)([MS])", c)]


@pytest.mark.parametrize("min_length,max_hits,secondary", [(1, 16, True), (10, 3, True), (20, 16, False), (10, 1, True)])
def test_model_lines_hold_against_the_text(case, min_length, max_hits, secondary):
    S, o = case
    text = S.text.tobytes()
    starts = dict(zip((n.encode() for n in S.doc_names), S.doc_starts))
    reads = _reads(S)
    quals = [bytes(33 + (j * 7 + i) % 40 for j in range(len(q))) for i, q in enumerate(reads)]
    seen = {"fwd": 0, "rev": 0, "unmapped": 0, "secondary": 0, "clipped": 0}
    for i, (q, ql) in enumerate(zip(reads, quals)):
        name = b"r%d" % i
        lines = SAM.read_lines(o, name, q, ql, min_length, max_hits, secondary)
        assert lines and all(l.endswith(b"\n") and l.count(b"\n") == 1 for l in lines)
        p = SAM.pick(o, q, min_length)
        for j, line in enumerate(lines, 1):
            f = line[:-1].split(b"\t")
            assert len(f) >= 11 and f[0] == name
            flag = int(f[1])
            if p is None:
                assert len(lines) == 1 and len(f) == 11 and flag == 4 and f[2:9] == [b"*", b"0", b"0", b"*", b"*", b"0", b"0"]
                assert f[9] == (q or b"*") and f[10] == (ql or b"*")
                seen["unmapped"] += 1
                continue
            lo, hi, k, a, b, rev = p
            occ = hi - lo + 1
            assert b - a >= min_length and len(lines) == (min(occ, max(max_hits, 1)) if secondary else 1)
            assert flag == (16 if rev else 0) | (256 if j > 1 else 0) and f[4] == b"255" and f[6:9] == [b"*", b"0", b"0"]
            assert f[11] == b"NH:i:%d" % occ and f[12] == b"HI:i:%d" % j and len(f) == 13
            ops = _parse_cigar(f[5])
            assert b"".join(b"%d%s" % x for x in ops) == f[5] and all(n > 0 for n, _ in ops) and [op for _, op in ops if op == b"M"] == [b"M"]
            searched = SAM.revcomp(q) if rev else q
            pos = starts[f[2]] + int(f[3]) - 1
            assert text[pos:pos + (b - a)] == searched[a:b]                  # the seed's own bases lie at POS of RNAME
            if j == 1:
                assert f[9] == searched and f[10] == (ql[::-1] if rev else ql)
                assert sum(n for n, _ in ops) == len(f[9])                   # CIGAR's query length
                assert ops == ([(a, b"S")] if a else []) + [(b - a, b"M")] + ([(len(q) - b, b"S")] if len(q) > b else [])
                seen["rev" if rev else "fwd"] += 1
                seen["clipped"] += 1 if a or len(q) > b else 0
            else:
                assert f[9] == b"*" and f[10] == b"*"
                seen["secondary"] += 1
        if p is not None and not secondary:
            assert len(lines) == 1
    assert seen["fwd"] > 5 and seen["rev"] > 5 and seen["unmapped"] >= 2 and seen["clipped"] > 5
    assert (seen["secondary"] > 0) == (secondary and max_hits > 1)


def test_model_strand_tie_goes_to_forward(case):
    """a read that is its own reverse complement matches on both strands with the same seed: forward is reported; a read whose reverse strand has the strictly longer
    seed is reported there"""
    S, o = case
    half = S.text[300:320].tobytes()
    pal = half + b"N" + SAM.revcomp(half)                                # its own reverse complement (the N stays): both strands hold the same seed
    assert SAM.revcomp(pal) == pal
    p = SAM.pick(o, pal, 10)
    assert p is not None and p[3:] == (0, 20, 0)
    line = SAM.read_lines(o, b"p", pal, None, 10, 1, False)[0].split(b"\t")
    assert int(line[1]) & 16 == 0 and line[5] == b"20M21S" and line[10] == b"*"
    q = SAM.revcomp(S.text[500:540].tobytes())
    assert SAM.pick(o, q, 20)[5] == 1 and SAM.pick(o, SAM.revcomp(q), 20)[5] == 0
    # an N is kept by the complement and ends a seed on both strands
    n = S.text[600:620].tobytes() + b"N" + S.text[621:650].tobytes()
    assert SAM.revcomp(n).count(b"N") == 1
    lo, hi, k, a, b, rev = SAM.pick(o, n, 10)
    assert (a, b, rev) == (21, 50, 0)


def test_model_header(case):
    S, o = case
    h = SAM.header(S.doc_names, S.doc_starts, S.n, b"@PG\tID:x\n")
    lines = h.split(b"\n")
    assert lines[0] == b"@HD\tVN:1.6\tSO:unsorted" and lines[-2] == b"@PG\tID:x" and lines[-1] == b""
    unit = S.L + S.pad
    assert lines[1:-2] == [b"@SQ\tSN:hap%d\tLN:%d" % (j, unit if j < S.H - 1 else S.n - j * unit) for j in range(S.H)]
    # starts given out of order: names stay in the given order, starts are sorted
    assert SAM.header(["a", "b"], [50, 0], 80) == b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:a\tLN:50\n@SQ\tSN:b\tLN:30\n"


def test_sam_binding_surface():
    """the ctypes wrapper has the two methods and binds their symbols; without a device the calls answer RBG_ENODEV / RBG_EARG, they do not crash"""
    import rowbowt_amd as ra
    from rowbowt_amd import capi
    for m in ("align_sam", "sam_header"):
        assert callable(getattr(ra.RowBowt, m)), m
    L = ra.lib()
    for f in ("rbg_align_sam", "rbg_sam_header"):
        assert f in capi.EXPORTS and getattr(L, f).argtypes is not None, f
    assert capi.SAM_SECONDARY == 1
    assert L.rbg_align_sam(None, None, None, None, None, None, None, None, None, 0, 20, 16, 0, None, None) == -3
    assert L.rbg_sam_header(None, None, None, None) == -4
