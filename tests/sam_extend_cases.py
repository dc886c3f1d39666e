"""Test infrastructure: the inputs the tests of the left extension share (tests/test_sam_extend_model.py checks on the CPU that they hold every kind of line
the GPU tests are meant to meet; tests/test_gpu_sam_extend.py and tests/test_gpu_extend_left.py run them on the device), and their classification by the
model.  The index is test_gpu_sam.py's toy pangenome: 5 haplotypes of 1 500 bases, 30 variant sites, documents hap0 .. hap4."""
import functools

import numpy as np

import orc
import sam_extend_model as XM
import sam_model as SAM
from synth import SynthIndex

TOY = dict(L=1500, H=5, n_sites=30, seed=23)
MIN_LENGTH, MAX_HITS = 20, 8


@functools.lru_cache(maxsize=None)
def toy():
    S = SynthIndex(**TOY)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    o.set_docs(S.doc_names, S.doc_starts)
    return S, o


def _sub(q, p):
    q[p] = ord("ACGT"[("ACGT".index(chr(q[p])) + 1) % 4])


def reads(S):
    """(name, read) pairs.  A window of the text with substitutions planted in its LEFT half has its longest seed right of them, so the walk meets them:
    one substitution (the whole prefix is taken), two far apart (a budget of 1 ends between them), a cluster (nothing is taken), one near the read's start
    (taken, then trimmed away), an N, a lower-case base; windows that start a few bases into a document behind foreign bases (the document's start ends the
    walk); windows over variant sites (the haplotypes that share the seed differ in the flank); half of everything reverse-complemented; exact and unmapped
    reads."""
    rng = np.random.default_rng(101)
    unit = S.L + S.pad
    out = []

    def window(h, s, m):
        return bytearray(S.text[h * unit + s:h * unit + s + m].tobytes())

    for i in range(40):
        h, s = i % S.H, int(rng.integers(40, S.L - 120))
        q = window(h, s, 100)
        kind = i % 8
        if kind == 0:
            _sub(q, int(rng.integers(8, 40)))
        elif kind == 1:
            p = int(rng.integers(25, 40))
            _sub(q, p)
            _sub(q, p - int(rng.integers(6, 15)))
        elif kind == 2:
            for p in (30, 28, 26, 23, 21, 18):
                _sub(q, p)
        elif kind == 3:
            _sub(q, 30)
            _sub(q, 30 - 6)
            q = q[22:]                                   # the second substitution two bases from the read's start
        elif kind == 4:
            _sub(q, 35)
            q[20] = ord("N")
        elif kind == 5:
            _sub(q, 33)
            q[12] = ord(chr(q[12]).lower())
        elif kind == 6:
            q = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), 14).tobytes()) + window(h, 0, 70)   # behind foreign bases, at a document's start
            _sub(q, 14 + 7)
        else:
            pass                                         # exact: a = 0
        out.append(bytes(q))
    for si, site in enumerate(S.sites):                  # a window with a variant site 12 bases left of a planted substitution
        site = int(site)
        if 30 <= site < S.L - 90 and si % 2 == 0:
            q = window(si % S.H, site - 15, 90)
            _sub(q, 15 + 12)
            out.append(bytes(q))
    out += [b"N" * 30, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 60).tobytes()), b""]
    out = [SAM.revcomp(q) if i % 2 else q for i, q in enumerate(out)]
    return [(b"x%d" % i, q) for i, q in enumerate(out)]


def quals(rs):
    return [bytes(33 + (j * 7 + i) % 60 for j in range(len(q))) for i, (_, q) in enumerate(rs)]


@functools.lru_cache(maxsize=None)
def records(K, secondary=True):
    """the model's records of the shared reads: per read the list XM.read_records gives"""
    S, o = toy()
    return [XM.read_records(o, q, MIN_LENGTH, MAX_HITS, secondary, K) for _, q in reads(S)]


def kinds(K):
    """which kinds of line the shared reads give at budget K"""
    seen = set()
    S, _ = toy()
    for (_, q), recs in zip(reads(S), records(K)):
        if recs == [None]:
            seen.add("unmapped")
            continue
        nms = set()
        for (lo, hi, k, a, b, rev), j, l, dn, offs, x in recs:
            e = x["ext"]
            seen.add("reverse" if rev else "forward")
            if a == 0:
                seen.add("a = 0")
            if a and e == a:
                seen.add("e = a")
            if 0 < e < a and x["why"] == "budget":
                seen.add("0 < e < a by the budget")
            if offs < a and x["steps"] == offs and x["why"] == "length":
                seen.add("cut by offs")
            if e == 0 and a > 0:
                seen.add("e = 0, a > 0")
            if len(x["mis"]) > x["nm"]:
                seen.add("trimmed a taken mismatch")
            s = SAM.revcomp(q) if rev else q
            if b"N" in s[a - x["steps"]:a] and x["steps"]:
                seen.add("N in the flank")
            nms.add(x["nm"])
        if len(recs) >= 2 and len(nms) >= 2:
            seen.add("secondary lines of different nm")
    return seen
