"""Positions at and across the width edges -- 2^31, the top of the 4-byte range, 2^32, 2^38 -- through everything that is built on locate: the
device locate chain with its order, document hits, SAM, the seed lists and toehold checkpoints, the markers at located positions, and the seed extensions:
FL, the LF and FL walks by themselves, the SAM lines extended to the left and on both sides.

Three run lists of 2 000 runs (gpu_common._random_run_index: the arrays define every answer, no text is needed):
  A  n = 2^32 - 17, the largest index with 4-byte positions;
  B  n = 2^32 - 16, the smallest with 8-byte positions (chosen by the load, no option set);
  C  2^38 < n < 2^40, 8-byte positions, values above 2^32 everywhere.
A and B are loaded on the run-indexed and on the slot layout (4096-row rank buckets and 256-position phi buckets: 0.4 GB on the device
at A, 0.7 GB at B), C on the run-indexed layout with the phi list and with phi slots.  Two rules hold for every call of this file: max_hits is finite (at
most 64: ranges of such an index are millions of rows wide), and the handles step one symbol at a time, without a jump table (the samples of a random
run list define toeholds for single-symbol steps only).

Every comparison is exact, against the oracle and the CPU models (sam_model, doc_hits_model, seeds_model, rb_locs_model, sam_extend_model, fl_model).  The
expected values are made by plain functions (expected(name) below: no device is touched; 5.3 s of CPU time for A, 6.1 s for B, 5.4 s for C), each leg's values in a function
of its own that also asserts, from the EXPECTED values, that the leg reaches the edges it is for (tests/test_wide_positions_expected.py runs them where no
GPU exists).

The extension legs read their reads off the models.  Reads that were walked hardly extend here -- a range is millions of rows wide, the primary line's row
is hi and not the row the read was walked from, so the clipped half of a substituted read meets another flank -- so a read is built from the row itself:
BWT[r], BWT[LF(r)], ... is what lies left of row r's position, the F bytes of the FL walk from r what lies right of it."""
import bisect
import contextlib
import functools
import types
from unittest import mock

import numpy as np
import pytest

import doc_hits_model as M
import fl_model as FM
import orc
import rowbowt_amd as ra
import sam_extend_model as XM
import sam_model as SAM
from rowbowt_amd import capi
from gpu_common import _lf_walk_reads, _pin_run_end_samples, _random_run_index, _random_run_index_exact, _with_layout, split
from rb_locs_model import loc_markers
from seeds_model import longest_seed, seeds_greedy, toehold_chkpnts
from test_gpu_loc_markers import _arrays, _want_at_locs
from test_rb_locs_model import mk, text_oracle

pytestmark = pytest.mark.gpu
MAXU = 2**64 - 1
EARG = -4
R = 2000
N_OF = {"A": 2**32 - 17, "B": 2**32 - 16}
POS_BYTES = {"A": 4, "B": 8, "C": 8}
# what the values of a leg must reach, per index: A the sign bit of a 32-bit word and the 2^16 values below the 32-bit sentinel; C 2^38
EDGES = {"A": (2**31, 2**32 - 2**16), "B": (2**31,), "C": (2**38,)}
SEEDS = {"A": 7101, "B": 7102, "C": 7103}
WIDE = ((capi.OPT_RANK_BUCKET_SHIFT, 12), (capi.OPT_PHI_BUCKET_SHIFT, 8))
# (layout, RBG_OPT_RUN_PHI, further options)
FORMS = {"A": ((capi.LAYOUT_RUNS, 0, ()), (capi.LAYOUT_SLOTS, 0, WIDE)), "B": ((capi.LAYOUT_RUNS, 0, ()), (capi.LAYOUT_SLOTS, 0, WIDE)),
         "C": ((capi.LAYOUT_RUNS, 1, ()), (capi.LAYOUT_RUNS, 2, ()))}
HITS = (1, 8, 64)            # every max_hits of the locate legs
MIN_LENGTH = 10
WALK_KS = (0, 4, 8)         # the budgets of the walks alone
SAM_KS = (0, 2, 4)          # ... and of the extended SAM lines


# ---- the CPU half: indices, reads, tables and every expected value --------------------------------------------------------------------------
def _reaches(name, what, values):
    v = np.asarray(values, dtype=np.uint64)
    for edge in EDGES[name]:
        assert (v >= np.uint64(edge)).any(), f"index {name}: no {what} at or above {edge}: the case this leg is about is missing"


def _run_list(name):
    """the run list of one index with the toeholds of the four one-symbol reads set on the document starts of the small table, and (A, B) a twentieth
    of the run-end samples within 2^15 of n"""
    rng = np.random.default_rng(SEEDS[name])
    if name == "C":
        heads, lens, ssa, esa, n = _random_run_index(rng, R, 500_000_000)
        assert (1 << 38) < n < (1 << 40)
        pins = {ord("A"): 2**32 - 1, ord("C"): 2**32, ord("G"): 2_000_000_001, ord("T"): 1_000_007}
    else:
        heads, lens, ssa, esa, n = _random_run_index_exact(rng, R, N_OF[name])
        pins = {ord("A"): 2**31 - 1, ord("C"): 2**31, ord("G"): n - 500, ord("T"): 1_000_007}
    _pin_run_end_samples(rng, heads, ssa, esa, n, top=0 if name == "C" else R // 20, toeholds=pins)
    return heads, lens, ssa, esa, n, pins, rng


def _tables(name, n, rng):
    """{"small": starts at the width edges below n, names of 0, 1 and 20 bytes; "large": 200 documents, the first at 0 (from 128 on: the locus order)}"""
    if name == "C":
        small = [0, 2_000_000_000, 2**32 - 1, 2**32, 300_000_000_000]
    else:
        small = [0, 2**31 - 1, 2**31, n - 1000]
    assert small == sorted(small) and small[-1] < n
    large = [0] + sorted(set(int(x) for x in rng.integers(1, n, 199)))
    assert len(large) == 200
    return {"small": (["", "a", "z" * 20, "d3", "d4"][:len(small)], small), "large": ([f"doc{j}" for j in range(200)], large)}


def _reads(o, heads, lens, n, rng):
    """300 reads that occur (LF walks of 1 to 60 symbols), 60 of them again with one substitution, 20 random ones, the empty read, one with an N, the
    four one-symbol reads -> (reads as walked, the same with every second one reverse-complemented)"""
    walk = _lf_walk_reads(o, heads, lens, n, rng, 300, 61)
    assert max(len(q) for q in walk) == 60
    sub = []
    for q in walk:
        if len(q) >= 24 and len(sub) < 60 and set(q) <= set(b"ACGT"):
            p = len(q) // 2
            sub.append(q[:p] + bytes([b"ACGT"[(b"ACGT".index(q[p]) + 1 + int(rng.integers(0, 3))) % 4]]) + q[p + 1:])
    assert len(sub) == 60
    rnd = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(rng.integers(1, 60)))) for _ in range(20)]
    body, tail = walk + sub + rnd, [b"", walk[0][-12:] + b"N" + walk[1][-20:], b"A", b"C", b"G", b"T"]
    return body + tail, [SAM.revcomp(q) if i % 2 else q for i, q in enumerate(body)] + tail


def _locate_values(E):
    """leg 1: ranges and toeholds of the reads as walked, a wrapped toehold (2^64 - 1) planted on two reads of several locations, the locations of every
    max_hits"""
    o = E.o
    E.seqs, E.off = ra.pack_reads(E.reads)
    E.wlo, E.whi, E.wk = o.find_range_w_toehold_batch(E.seqs, E.off)
    matched = E.whi >= E.wlo
    occ = np.where(matched, E.whi - E.wlo + np.uint64(1), np.uint64(0))
    assert int(matched.sum()) >= 300 and int(occ.max()) > 1_000_000
    for c, t in E.pins.items():     # the one-symbol reads have the toeholds the run list was given
        assert o.find_range_w_toehold(bytes([c]))[2] == t
    E.multi = np.flatnonzero(occ >= 3)[:2]
    assert len(E.multi) == 2
    E.wk_planted = E.wk.copy()
    E.wk_planted[E.multi] = np.uint64(MAXU)
    E.locs = {mh: o.locs_at_batch(E.wlo, E.whi, E.wk_planted, mh) for mh in HITS}
    E.locs_unplanted = o.locs_at_batch(E.wlo, E.whi, E.wk, 8)
    real = E.locs[64][1][E.locs[64][1] != np.uint64(MAXU)]
    assert (E.locs[64][1] == np.uint64(MAXU)).sum() == 2 and int(real.max()) < E.n
    _reaches(E.name, "row of a range", np.concatenate([E.wlo[matched], E.whi[matched]]))
    _reaches(E.name, "toehold", E.wk[matched])
    _reaches(E.name, "location", real)
    if E.name == "A":   # real toeholds next to the 32-bit key of the wrapped one (k_locate.hip k_keys32): within 2^16 of 0xFFFFFFFF
        assert ((E.wk[matched] > np.uint64(0xFFFFFFFF - 2**16)) & (E.wk[matched] < np.uint64(E.n))).any()


def _oracle_resolve(E, table, locs):
    """the oracle's resolve_offset of every position -> (doc, offset) in the model's terms, and the model held to it"""
    names, starts = E.tables[table]
    E.o.set_docs(names, starts)
    index = {nm.encode(): j for j, nm in enumerate(names)}
    doc, off = M.resolve(locs, starts)
    for l, d, f in zip(locs.tolist(), doc.tolist(), off.tolist()):
        nm, wf = SAM.resolve_offset(E.o, l)                                   # (bytes, or None: an empty name is a name)
        assert (d, f) == ((M.DOC_NONE, l) if nm is None else (index[nm], wf)), (table, l)
    return doc, off


def _doc_values(E):
    """leg 2: the model's outputs over the locations of leg 1 (with the planted toeholds: the device calls) and over those of the reads' own toeholds
    (the host call, which searches itself), under both tables; doc and offset of every distinct location, from the oracle"""
    E.uniq = np.unique(np.concatenate([E.locs[64][1], np.array([0, E.n - 1, MAXU], np.uint64)]))
    E.docs, E.resolved = {}, {}
    for table, (names, starts) in E.tables.items():
        E.resolved[table] = _oracle_resolve(E, table, E.uniq)
        for key, (woff, wlocs) in (("dev", E.locs[8]), ("dev64", E.locs[64]), ("host", E.locs_unplanted)):
            sets, ndocs, nodoc, doc_reads = M.doc_hits(wlocs, woff, starts)
            doc = M.resolve(wlocs, starts)[0]
            doc_locs = np.bincount(doc[doc != M.DOC_NONE].astype(np.int64), minlength=len(starts)).astype(np.uint64)
            E.docs[table, key] = {"sets": sets, "ndocs": ndocs, "nodoc": nodoc, "doc_reads": doc_reads, "doc_locs": doc_locs}
        assert int(E.docs[table, "dev"]["nodoc"][E.multi].min()) >= 1            # the wrapped toeholds have no document
    for key in ("dev", "host"):
        assert (E.docs["small", key]["doc_locs"] > 0).all(), "a document of the small table receives no location"
    assert int(E.docs["large", "dev"]["ndocs"].max()) >= 2
    if E.name == "C":
        doc, off = E.resolved["small"]
        assert int(off[doc != M.DOC_NONE].max()) >= 10**9, "no offset inside a document of ten digits"
    # the bound the chunked host call is given: the batch has several times as many locations, on many reads
    E.chunk_locs = 100
    assert int(E.locs_unplanted[0][-1]) > 4 * E.chunk_locs and int((np.diff(E.locs_unplanted[0].astype(np.int64)) > 0).sum()) > 100


def _quals(reads):
    return [bytes(33 + (j * 5 + i) % 60 for j in range(len(q))) for i, q in enumerate(reads)]


def _sam_values(E):
    """leg 3: the model's lines of every call the test makes"""
    o = E.o
    E.names = [b"r%d" % i for i in range(len(E.sam_reads))]
    E.quals = _quals(E.sam_reads)
    E.sam, E.header = {}, {}
    flags, pos_widths, nh = set(), set(), 0
    for table, (names, starts) in E.tables.items():
        o.set_docs(names, starts)
        E.header[table] = SAM.header(names, starts, E.n)
        for secondary in (False, True):
            for max_hits in (1, 8):
                for ql in (True, False):
                    want = SAM.lines(o, E.names, E.sam_reads, E.quals if ql else None, MIN_LENGTH, max_hits, secondary)
                    assert want is not None
                    E.sam[table, secondary, max_hits, ql] = b"".join(want)
                    f = [l[:-1].split(b"\t") for l in want]
                    flags |= {int(x[1]) for x in f}
                    if table == "small":
                        pos_widths |= {len(x[3]) for x in f if x[1] != b"4"}
                    nh = max([nh] + [int(x[11][5:]) for x in f if x[1] != b"4"])
        # min_length 1: the one-symbol reads map, at the document starts the run list pins their toeholds on (POS 1)
        want = SAM.lines(o, E.names, E.sam_reads, None, 1, 8, True)
        E.sam[table, "min_length 1"] = b"".join(want)
        if table == "small":
            pos1 = sum(1 for l in want[-8 * 4:] if l.split(b"\t")[3] == b"1" and l.split(b"\t")[1] in (b"0", b"16"))
            assert pos1 >= 2, "the one-symbol reads do not map at the starts of the small table's documents"
    assert flags == {0, 4, 16, 256, 272}, flags
    assert nh >= 10**6, nh
    if E.name == "C":
        assert {10, 11, 12} <= pos_widths, pos_widths
        assert any(len(l.split(b"LN:")[1]) > 10 for l in E.header["small"].splitlines() if b"LN:" in l)   # (an LN above 2^32)


def _seed_values(E):
    """leg 4: seed lists, longest seeds, checkpoints and greedy locations of 150 reads -- occurring ones, substituted ones, reverse complements"""
    o = E.o
    top = np.flatnonzero((E.whi >= E.wlo) & (E.wk >= np.uint64(EDGES[E.name][-1])) & (E.wk < np.uint64(E.n - 100)) & (np.diff(E.off) >= np.uint64(MIN_LENGTH)))
    assert len(top) >= 3
    E.seed_reads = E.reads[:60] + E.sam_reads[1:60:2] + E.reads[300:330] + E.reads[-30:] + [E.reads[i] for i in top[:6]]
    E.seeds = {(ml, ws): [seeds_greedy(o, q, ml, ws) for q in E.seed_reads] for ml in (0, MIN_LENGTH) for ws in (True, False)}
    E.longest = {ml: [longest_seed(seeds_greedy(o, q, ml)) or (1, 0, 0, 0, 0) for q in E.seed_reads] for ml in (0, MIN_LENGTH, 40)}
    E.chk = {w: [toehold_chkpnts(o, q, w) for q in E.seed_reads] for w in (1, 7, 20)}
    E.greedy_locs = [o.greedy_locate(q, MIN_LENGTH, 8)[0] for q in E.seed_reads]
    recs = [r for ml in (0, MIN_LENGTH) for l in E.seeds[ml, True] for r in l if r[1] >= r[0]]
    assert sum(len(l) >= 2 for l in E.seeds[MIN_LENGTH, True]) >= 20 and any(w == (1, 0, 0, 0, 0) for w in E.longest[40])
    _reaches(E.name, "row of a seed's range", [r[1] for r in recs])
    _reaches(E.name, "toehold of a seed", [r[4] for r in recs if r[4] < E.n])
    chk = [r for w in E.chk for l in E.chk[w] for r in l]
    assert len(chk) > 1000
    _reaches(E.name, "toehold of a checkpoint", [r[4] for r in chk if r[4] < E.n])
    _reaches(E.name, "greedy location", [x for l in E.greedy_locs for x in l if x < E.n])


def _marker_values(E):
    """leg 5: a text-position table whose runs are taken from the locations of leg 1 -- runs that start at one, end at one, straddle 2^31 and (C) 2^32,
    one that ends at n - 1 -- over a grid of 3 000 runs that covers half of [0, n); a value's position field is its run's start (below 2^48)"""
    n = E.n
    woff, wlocs = E.locs[8]
    U = np.unique(wlocs[wlocs < np.uint64(n - 100)]).tolist()
    special = [(2**31 - 3, 2**31 + 3), (n - 6, n - 1)] + ([(2**32 - 3, 2**32 + 3)] if n > 2**32 + 3 else [])
    special += [(l - 2, l + 2) for l in U if l >= EDGES[E.name][-1]][:200]                    # (on A: the locations within 2^16 of 2^32)
    special += [(l, l + 5) for l in U[5::40]] + [(l - 7, l) for l in U[25::40] if l >= 7]
    step = n // 3000
    grid = [(s, s + step // 2) for s in range(step // 3, n - step, step)]
    runs = []
    for s, e in special:                     # (in this order: a run that overlaps one already taken is left out)
        if all(e < a or s > b for a, b in runs):
            runs.append((s, e))
    runs.sort()
    begins = [a for a, _ in runs]
    for s, e in grid:
        j = bisect.bisect_right(begins, e) - 1                                               # the last special run that starts at or before e
        if j < 0 or runs[j][1] < s:
            runs.append((s, e))
    runs.sort()
    assert all(runs[j][1] < runs[j + 1][0] for j in range(len(runs) - 1)) and runs[-1][1] <= n - 1 and len(runs) > 3000
    assert (n - 6, n - 1) in runs and (2**31 - 3, 2**31 + 3) in runs
    E.mk_runs = [(s, e, [mk(j % 7, s, (j + t) % 3) for t in range(1 + j % 3)]) for j, (s, e) in enumerate(runs)]
    E.ot = text_oracle(E.mk_runs)
    E.mk_at_locs = _want_at_locs(E.ot, wlocs, woff, E.off)
    E.loc_mk = [loc_markers(E.o, E.ot, q, MIN_LENGTH, 8) for q in E.seed_reads]
    lens = np.diff(E.off).astype(np.int64)
    per_loc = [len(E.ot.markers_at(int(l), (int(l) + int(lens[i]) - 1) & MAXU)) for i in range(len(lens)) for l in wlocs[int(woff[i]):int(woff[i + 1])]]
    assert 0 in per_loc and sum(1 for c in per_loc if c) > 200, "every location hits a run, or hardly any does"
    hit = [v & (2**48 - 1) for l in E.mk_at_locs for v in l]
    _reaches(E.name, "run that is hit", hit)
    _reaches(E.name, "run hit through the greedy locations", [v & (2**48 - 1) for w in E.loc_mk for v in w[1]])


# ---- the two extension legs: walks read off the models, reads built from a line's own row -----------------------------------------------------
class _Memo:
    """the oracle with its pure queries remembered: the models ask the same ones again for every call that is expected (the document table is not
    among them: resolve_offset goes to the oracle itself)"""

    def __init__(self, o):
        self.h, self.L, self.n = o.h, o.L, o.n
        self.LF, self.access, self.find_range_w_toehold = (functools.lru_cache(maxsize=None)(f) for f in (o.LF, o.access, o.find_range_w_toehold))
        self._locs = functools.lru_cache(maxsize=None)(lambda lo, hi, k, mh: tuple(o.locs_at(lo, hi, k, mh)))

    def locs_at(self, lo, hi, k, max_hits=MAXU):
        return list(self._locs(lo, hi, k, max_hits))


def _other(c, d):
    """another base than c (d = 1, 2, 3)"""
    return b"ACGT"[(b"ACGT".index(c) + d) % 4]


def _left_flank(o, r, L):
    """BWT[r], BWT[LF(r)], ...: the up to L bases left of row r's position, nearest first, and the rows they are read at (it ends at the terminator)"""
    out, rows = bytearray(), []
    while len(out) < L:
        c = o.access(r)
        if c not in b"ACGT":
            break
        out.append(c)
        rows.append(r)
        r = o.LF(r, r, c)[0]
    return bytes(out), rows


def _right_flank(fl, r, skip, L):
    """the F bytes of the FL walk from row r after `skip` steps: the up to L bases from `skip` positions right of row r's position on, and their rows;
    None when a skipped row has no base"""
    for _ in range(skip):
        c, r = fl.step(r)
        if not c:
            return None, []
    out, rows = bytearray(), []
    while len(out) < L:
        c, nr = fl.step(r)
        if not c:
            break
        out.append(c)
        rows.append(r)
        r = nr
    return bytes(out), rows


def _lf_chain(o, r, k):
    """LF^k(r), or None when the terminator is on the way"""
    for _ in range(k):
        c = o.access(r)
        if c not in b"ACGT":
            return None
        r = o.LF(r, r, c)[0]
    return r


def _fl_chain(fl, r, k):
    for _ in range(k):
        c, r = fl.step(r)
        if not c:
            return None
    return r


def _crossings(name, rows):
    """{(edge, upwards)} for every edge that the rows of one walk cross in the order visited: a row below it and a LATER one at or above it, or the reverse"""
    out = set()
    for edge in EDGES[name]:
        above = [r >= edge for r in rows]
        if True in above and False in above[above.index(True):]:
            out.add((edge, False))
        if False in above and True in above[above.index(False):]:
            out.add((edge, True))
    return out


def _plant(body, lo, hi, j, rng):
    """j % 11 substitutions at random places of body[lo:hi] (in place)"""
    for p in rng.choice(hi - lo, min(j % 11, hi - lo), replace=False):
        body[lo + int(p)] = _other(body[lo + int(p)], 1 + j % 3)


def _extend_values(E):
    """leg 6: items of rbg_extend_left_dev and rbg_extend_right_dev -- a row, the row's own flank read off the models with 0 to 10 substitutions, a skip, a
    limit -- at the width edges, at rows whose walks cross an edge on their way, at rows whose walks meet "no base"; the rows of rbg_fl_dev"""
    o, fl, n, name = E.xo, E.fl, E.n, E.name
    rng = np.random.default_rng(SEEDS[name] + 50)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    rows = [0, 1, n - 1] + [e - d for e in EDGES[name] for d in (1, 0)] + ([2**32 + d for d in (-40, -1, 0, 1, 40)] if name == "C" else [])
    rows += [int(v) for v in rng.integers(0, n, 300)]
    generic = [dict(row=r) for r in rows]
    # rows found by search: the walk from FL^k(z) (left) or LF^k(z) (right) reaches z after k steps; z at or above an edge and the start below it, and the
    # reverse (z below, the start above).  Such walks get a long flank, the whole limit and at most two substitutions, so that they arrive.
    zone = {e: [int(v) for v in rng.integers(e, n, 12)] + [int(v) for v in rng.integers(max(e - 2**20, 0), e, 12)] for e in EDGES[name]}
    term = int(E.lens[:int(np.flatnonzero(E.heads == 1)[0])].sum())
    assert o.access(term) == 1 and fl.step(0) == (0, FM.NONE)
    E.left, E.right = {}, {}
    for side, items in (("left", E.left), ("right", E.right)):
        chain = (lambda r, k: _fl_chain(fl, r, k)) if side == "left" else (lambda r, k: _lf_chain(o, r, k))
        spec = list(generic)
        for e, zs in zone.items():
            for i, z in enumerate(zs):
                k = 2 + 3 * (i % 6)
                spec.append(dict(row=z, far=k, z=z, edge=e))           # (the start is resolved below: a right item's skip goes on top of k)
        # the walk ends on "no base": k steps after the start, at the terminator (left, BWT[term]) or at row 0 (right, whose F byte is the terminator)
        end = term if side == "left" else 0
        spec += [dict(row=end, far=k, z=end, nobase=True) for k in (0, 1, 5, 30)]
        if side == "right":
            spec += [dict(row=0, far=k, z=0, nobase=True, into=True) for k in (0, 1, 5, 30)]   # ... and a skip that itself meets row 0: the zero record
        seqs, pos, row_, skip_, lim_, frows = [], [], [], [], [], []
        for j, it in enumerate(spec):
            tail = 10 + (j * 11) % 61                                  # the compared bases: 10 .. 70
            skip = (j * 7) % 61 if side == "right" else 0              # 0 .. 60, neighbours far apart
            row = it["row"]
            if "far" in it:
                tail = max(tail, it["far"] + 12)
                if it.get("into"):
                    skip, row = it["far"] + 1 + j % 3, chain(it["z"], it["far"])
                else:
                    row = chain(it["z"], it["far"] + skip)
                assert row is not None, (side, it)
            if side == "left":
                ref, at = _left_flank(o, row, tail)
            else:
                ref, at = _right_flank(fl, row, skip, tail)
                ref = ref or b""
            body = bytearray(ref) + bytearray(rng.choice(acgt, tail - len(ref)).tobytes())      # (beyond "no base": any bases)
            if "far" in it:
                for p in rng.choice(np.arange(it["far"] + 2, tail), j % 3, replace=False):
                    body[int(p)] = _other(body[int(p)], 1 + j % 3)
                limit = 2**40
            else:
                _plant(body, 0, tail, j, rng)
                if j % 13 == 5:
                    body[3] = ord("N")
                if j % 17 == 3:
                    body[6] = ord(chr(body[6]).lower())
                limit = (0, 1, tail, tail + 5, 2**33, 2**40)[j % 6]
            if side == "left":                                         # the flank reversed, then six bases that no walk reads
                seqs.append(bytes(body[::-1]) + bytes(rng.choice(acgt, 6).tobytes()))
                pos.append(tail)
            else:                                                      # b bases that no walk reads (b >= skip), then the flank
                b = skip + j % 4
                seqs.append(bytes(rng.choice(acgt, b).tobytes()) + bytes(body))
                pos.append(b)
            row_.append(row)
            skip_.append(skip)
            lim_.append(limit)
            frows.append(at)
        perm = rng.permutation(len(seqs))                              # item j reads sequence perm[j]
        items["packed"], items["off"] = ra.pack_reads([seqs[j] for j in np.argsort(perm)])
        items.update(seq=perm.astype(np.uint32), pos=np.array(pos, np.uint32), row=np.array(row_, np.uint64), skip=np.array(skip_, np.uint32),
                     limit=np.array(lim_, np.uint64), want={})
        for K in WALK_KS:
            if side == "left":
                items["want"][K] = [XM.extend(o, seqs[j], pos[j], row_[j], lim_[j], K) for j in range(len(seqs))]
            else:
                items["want"][K] = [FM.extend_right(fl, seqs[j], pos[j], row_[j], skip_[j], lim_[j], K) for j in range(len(seqs))]
        # what the expected walks reach
        ends = {"length", "budget", "base"} | ({"skip"} if side == "right" else set())
        visited, crossed = [], []
        for K in WALK_KS:
            w = items["want"][K]
            assert {x["why"] for x in w} == ends, (side, K, {x["why"] for x in w})
            assert max(len(x["mis"]) for x in w) == K
            visited += [r for x, at in zip(w, frows) for r in at[:x["steps"]]]
            crossed += [_crossings(name, at[:x["steps"]]) for x, at in zip(w, frows)]
        assert any(len(x["mis"]) > x["nm"] for x in items["want"][8]), "no record with trimmed mismatches"
        _reaches(name, f"row of a {side} walk", visited)
        assert sum(1 for c in crossed if c) >= 20
        # (both ways over the first edge; the top 2^16 rows of A lie in its last run, a run of T: LF and FL map those rows to themselves, no walk enters or
        # leaves them, and the walks that start there stay -- they are the ones that reach that edge)
        assert set().union(*crossed) >= {(EDGES[name][0], up) for up in (False, True)}, (side, set().union(*crossed))
        for it, x in zip(spec, items["want"][8]):                      # the "no base" items end where they were aimed
            if it.get("nobase"):
                assert (x["why"], x["steps"]) == (("skip", 0) if it.get("into") else ("base", it["far"])), (side, it, x)
        assert {int(v) for v in items["limit"]} >= {0, 1, 2**33, 2**40} and (side == "left" or int(np.abs(np.diff(items["skip"][:64].astype(np.int64))).min()) >= 7)
    # FL rows: those of the items, the first and last row of every base's F interval, rows whose FL value is a zone row
    fr = set(int(r) for r in E.left["row"]) | set(int(r) for r in E.right["row"])
    for c in b"ACGT":
        fr |= {fl.F[c], fl.F[c] + fl.count[c] - 1}
    fr |= {_lf_chain(o, z, 1) for zs in zone.values() for z in zs} - {None}
    E.fl_rows = np.array(sorted(fr), np.uint64)
    want = [fl.step(int(r)) for r in E.fl_rows]
    E.fl_sym, E.fl_next = np.array([w[0] for w in want], np.uint8), np.array([w[1] for w in want], np.uint64)
    base = E.fl_sym != 0
    assert (~base).any() and (E.fl_next[~base] == np.uint64(MAXU)).all() and int(E.fl_next[base].max()) < n
    _reaches(name, "row given to FL", E.fl_rows)
    _reaches(name, "FL value", E.fl_next[base])
    if name == "C":                                                    # FL values above 2^32 from rows below it, and the reverse
        assert ((E.fl_rows < 2**32) & base & (E.fl_next >= 2**32)).any() and ((E.fl_rows >= 2**32) & base & (E.fl_next < 2**32)).any()
    else:                                                              # A, and B (n = 2^32 - 16: no value of B reaches 2^32): the 2^16 values below 2^32
        assert (E.fl_next[base] >= 2**32 - 2**16).any() and (E.fl_rows >= 2**32 - 2**16).any()


def _ext_kinds(reads, recs, starts, n, K):
    """test_gpu_sam_extend_both.kinds over records of read_records_both, with the left walk's kinds and those of the limits"""
    seen, last, srt = set(), max(starts), sorted(starts)
    for q, rr in zip(reads, recs):
        if rr == [None]:
            continue
        m = len(q)
        for (lo, hi, k, a, b, rev), j, l, dn, offs, x, y in rr:
            if x["ext"] > 0:
                seen.add("left clip moved")
            if m > b and y["ext"] == m - b:
                seen.add("right clip gone")
            if m > b and 0 < y["ext"] < m - b:
                seen.add("right clip shortened")
            if x["ext"] > 0 and y["ext"] > 0:
                seen.add("both clips moved")
            if x["nm"] > 0 and y["nm"] > 0 and x["nm"] + y["nm"] == K:
                seen.add("budget split")
            if rev and y["ext"] > 0:
                seen.add("reverse")
            if x["why"] == "length" and x["steps"] < a:
                seen.add("cut by the document's start")
            if y["why"] == "length" and y["steps"] < m - b:
                seen.add("cut by the document's end")
            if y["ext"] > 0 and l - offs == last:
                seen.add("a right walk in the last document")
            if offs >= 2**32 and x["steps"] > offs % 2**32:
                seen.add("a left limit above 2^32 whose low word would end the walk")
            limit = (srt[bisect.bisect_right(srt, l)] if l - offs != last else n) - (l + b - a)
            if limit >= 2**32 and y["steps"] > limit % 2**32:
                seen.add("a right limit above 2^32 whose low word would end the walk")
    return seen


def _sam_extend_texts(E, seen, lines):
    """the model's text of every call of leg 7 into E.x_sam; the kinds of line into seen[K], (row, location, offset, left record, right record) of every line
    at K = 4 into lines"""
    o, fl = E.xo, E.fl
    for table, (names, starts) in E.x_tables.items():
        E.o.set_docs(names, starts)
        for K in SAM_KS:
            ql = E.x_quals if K == 4 else None
            for secondary in (False, True):
                for max_hits in (1, 8):
                    E.x_sam[table, False, secondary, max_hits, K] = XM.text(o, E.x_names, E.x_reads, ql, MIN_LENGTH, max_hits, secondary, K)
                    both = FM.lines_both(o, fl, starts, E.x_names, E.x_reads, ql, MIN_LENGTH, max_hits, secondary, K)
                    assert both is not None
                    E.x_sam[table, True, secondary, max_hits, K] = b"".join(both)
            if K:
                recs = [FM.read_records_both(o, fl, starts, q, MIN_LENGTH, 8, True, K) for q in E.x_reads]
                kinds = _ext_kinds(E.x_reads, recs, starts, E.n, K)
                seen[K] |= kinds
                if table == "cut":
                    assert {"cut by the document's start", "cut by the document's end"} <= kinds, kinds
                if K == 4:
                    lines += [(hi - (j - 1), l, offs, x, y) for rr in recs if rr != [None] for (lo, hi, k, a, b, rev), j, l, dn, offs, x, y in rr]


def _sam_extend_values(E):
    """leg 7: the reads of leg 3 and 150 reads built from a line's own row -- the row's left flank reversed, a seed, its right flank, the base nearest the seed
    replaced on either side --, under the two tables and a third cut from the constructed reads' locations; the model's text of every call"""
    o, fl, n, name = E.xo, E.fl, E.n, E.name
    rng = np.random.default_rng(SEEDS[name] + 60)
    top = EDGES[name][-1]
    # seeds: what the FL walk of 28 to 40 steps from a row z spells (z is then a row of its range); a quarter of the z at or above the last edge
    cand = []
    for i in range(900):
        z = int(rng.integers(top, n)) if i % 4 == 0 else int(rng.integers(0, n))
        m = int(rng.integers(28, 41))
        s, _ = _right_flank(fl, z, 0, m)
        if s is not None and len(s) == m:
            cand.append(s)
    seqs, off = ra.pack_reads(cand)
    clo, chi, ck = E.o.find_range_w_toehold_batch(seqs, off)
    assert (chi >= clo).all()
    first = np.flatnonzero((ck >= np.uint64(top)) & (ck < np.uint64(n - 100)))                # toeholds at or above the last edge first, as leg 4's `top`
    order = first.tolist()[:50] + [i for i in range(len(cand)) if i not in set(first.tolist()[:50])]
    assert len(first) >= 10
    built = []                                                         # (read as given, lo, hi, seed length, primary location)
    for i in order:
        if len(built) == 150:
            break
        s, lo, hi, k = cand[i], int(clo[i]), int(chi[i]), int(ck[i])
        t = len(built)
        r = hi - 2 if t % 4 == 3 and hi - lo >= 2 else hi
        left, _ = _left_flank(o, r, int(rng.integers(8, 20)))
        right, _ = _right_flank(fl, r, len(s), int(rng.integers(8, 20)))
        if right is None or min(len(left), len(right)) < 8:
            continue
        for d in (1, 2, 3):                                            # up to three choices of the replaced bases: the seed must stay the read's pick
            lf, rt = bytearray(left), bytearray(right)
            lf[0], rt[0] = _other(lf[0], d), _other(rt[0], 1 + (d + t) % 3)
            if t % 5 == 0:
                rt[-1] = _other(rt[-1], d)                             # (the right clip is shortened, not gone)
            read = bytes(lf[::-1]) + s + bytes(rt)
            given = SAM.revcomp(read) if t % 2 else read
            p = SAM.pick(o, given, MIN_LENGTH)
            if p is not None and (p[0], p[1], p[3], p[4], p[5]) == (lo, hi, len(lf), len(lf) + len(s), t % 2):
                built.append((given, lo, hi, len(s), o.locs_at(lo, hi, p[2], 1)[0]))
                break
    assert len(built) == 150, len(built)
    E.x_reads = list(E.sam_reads) + [b[0] for b in built]
    E.x_names = [b"x%d" % i for i in range(len(E.x_reads))]
    E.x_quals = _quals(E.x_reads)
    # the third table: a document starts 3 positions before a third of the locations, 2 positions after the seed's end of another third
    cut = {0}
    for t, (_, lo, hi, sl, l) in enumerate(built):
        if t % 3 == 0 and l >= 3:
            cut.add(l - 3)
        elif t % 3 == 1 and l + sl + 2 < n:
            cut.add(l + sl + 2)
    cut = sorted(cut)
    if n > 2**33:              # C: limits above 2^32 whose low word alone would cut the walk short -- a document that starts 2^32 + 3 positions before the
        for t, (_, lo, hi, sl, l) in enumerate(built):                 # location and the next one 2^32 + 2 positions after the seed's end, no start between them
            before, after = l - 2**32 - 3, l + sl + 2 + 2**32
            if t % 3 == 2 and before > 0 and after < n and bisect.bisect_left(cut, before) == bisect.bisect_left(cut, after):
                cut = sorted(set(cut) | {before, after})
    assert 60 < len(cut) < capi.DOCS_MAX // 100 and cut[-1] < n
    E.x_tables = dict(E.tables, cut=([f"c{j}" for j in range(len(cut))], cut))
    E.x_sam, seen, lines = {}, {K: set() for K in SAM_KS}, []
    with mock.patch.object(SAM, "pick", functools.lru_cache(maxsize=None)(SAM.pick)):       # (a read's pick is the same in every call: the models' own, remembered)
        _sam_extend_texts(E, seen, lines)
    assert seen[4] >= {"left clip moved", "right clip gone", "right clip shortened", "both clips moved", "reverse", "cut by the document's start",
                       "cut by the document's end", "a right walk in the last document"}, seen[4]
    assert "budget split" in seen[2], seen[2]
    if name == "C":
        assert {"a left limit above 2^32 whose low word would end the walk", "a right limit above 2^32 whose low word would end the walk"} <= seen[4], seen[4]
    per = len(E.x_tables)                                              # (every table gives the same walks but for the cuts: count the lines of one table)
    for side, pick in (("left", 3), ("right", 4)):
        ext = [ln for ln in lines if ln[pick]["ext"] > 0 and ln[pick]["nm"] > 0]
        assert len(ext) >= 100 * per, (side, len(ext))
        _reaches(name, f"row of a line extended to the {side}", [ln[0] for ln in ext])
        _reaches(name, f"location of a line extended to the {side}", [ln[1] for ln in ext])
    if name == "C":
        assert any(x["ext"] > 0 and offs + 1 - x["ext"] >= 10**10 for _, _, offs, x, _ in lines), "no extended line whose POS has 11 digits"


@functools.lru_cache(maxsize=None)
def expected(name):
    """everything the legs compare against, for index "A", "B" or "C"; nothing here touches a device"""
    E = types.SimpleNamespace(name=name)
    E.heads, E.lens, E.ssa, E.esa, E.n, E.pins, rng = _run_list(name)
    E.o = orc.Oracle.from_runs(E.heads, E.lens, E.ssa, E.esa)
    E.tables = _tables(name, E.n, rng)
    E.reads, E.sam_reads = _reads(E.o, E.heads, E.lens, E.n, rng)
    _locate_values(E)
    _doc_values(E)
    _sam_values(E)
    _seed_values(E)
    _marker_values(E)
    E.fl, E.xo = FM.FL(E.heads, E.lens), _Memo(E.o)
    E.fl.step = functools.lru_cache(maxsize=None)(E.fl.step)
    _extend_values(E)
    _sam_extend_values(E)
    return E


# ---- the device half ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def indices():
    """expected(name), made when the first handle of an index asks for it and kept for the second"""
    made = {}
    yield lambda name: made.setdefault(name, expected(name))
    for E in made.values():
        E.o.close()
        E.ot.close()
    expected.cache_clear()


@pytest.fixture(scope="module", params=["A-runs", "A-slots", "B-runs", "B-slots", "C-philist", "C-phislots"])
def case(request, indices):
    """one handle of an index: single-symbol steps, no jump table; A and B on both layouts, C with the phi list and with phi slots"""
    import time
    E = indices(request.param[0])
    layout, phi, more = FORMS[E.name][0 if request.param.endswith(("runs", "philist")) else 1]
    t0 = time.perf_counter()
    with contextlib.ExitStack() as st:
        for opt, v in ((capi.OPT_KMER_STEPS, 1), (capi.OPT_JUMP_K, 0), (capi.OPT_RUN_PHI, phi)) + tuple(more):
            st.enter_context(capi.default_option(opt, v))
        rb = _with_layout(layout, lambda: ra.RowBowt.from_runs(E.heads, E.lens, E.ssa, E.esa, device=0))
    i = rb.info()
    print(f"index {E.name}, layout {layout}, phi {phi}: loaded in {time.perf_counter() - t0:.2f} s, {i.hbm_bytes / 1e6:.0f} MB on the device")
    assert i.n == E.n and i.pos_bytes == POS_BYTES[E.name] and i.rank_layout == layout and i.kmer_steps == 1
    yield E, rb
    rb.close()


def _set_docs(E, rb, table):
    names, starts = E.tables[table]
    rb.set_docs(names, starts)
    rb.docs_prepare()
    return names, starts


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}[a.dtype])).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


class _Chain:
    """rbg_find_range_w_toehold_dev, then plan, order and fill with the order, on buffers that stay on the device"""

    def __init__(self, E, rb):
        import torch
        self.E, self.rb, self.L, self.N = E, rb, ra.lib(), len(E.reads)
        self.st = torch.cuda.current_stream().cuda_stream
        N, L = self.N, self.L
        d_seqs = torch.from_numpy(np.concatenate([E.seqs, np.zeros((-len(E.seqs)) % 16 + 16, np.uint8)])).cuda()
        d_off = _t(E.off)
        self.d_lo, self.d_hi, self.d_k = (torch.empty(N, dtype=torch.int64, device="cuda") for _ in range(3))
        assert L.rbg_find_range_w_toehold_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, self.d_lo.data_ptr(), self.d_hi.data_ptr(), self.d_k.data_ptr(), self.st) == 0
        torch.cuda.synchronize()
        assert (_u64(self.d_lo) == E.wlo).all() and (_u64(self.d_hi) == E.whi).all() and (_u64(self.d_k) == E.wk).all()
        self.d_k.copy_(torch.from_numpy(E.wk_planted.view(np.int64)))
        self.d_loc_off = torch.empty(N + 1, dtype=torch.int64, device="cuda")
        self.tmp_bytes, self.ws_bytes = L.rbg_locate_plan_tmp_bytes(N), L.rbg_locate_order_ws_bytes(N)
        self.d_tmp = torch.empty(self.tmp_bytes, dtype=torch.uint8, device="cuda")
        self.d_ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda")

    def args(self, mh):
        return (self.rb.h, self.d_lo.data_ptr(), self.d_hi.data_ptr(), self.d_k.data_ptr(), self.N, mh, self.d_loc_off.data_ptr())

    def located(self, mh, fill32=False):
        """-> (loc_off, locations still on the device, the order's permutation); one guard element behind the locations"""
        import torch
        L, N, rb = self.L, self.N, self.rb
        assert L.rbg_locate_plan_dev(rb.h, self.d_lo.data_ptr(), self.d_hi.data_ptr(), N, mh, self.d_loc_off.data_ptr(), self.d_tmp.data_ptr(), self.tmp_bytes, self.st) == 0
        total = int(self.d_loc_off[-1].item())
        assert total == int(self.E.locs[mh][0][-1])
        assert L.rbg_locate_order_dev(rb.h, self.d_k.data_ptr(), N, self.d_ws.data_ptr(), self.ws_bytes, self.st) == 0
        d_locs = torch.full((total + 1,), -7, dtype=torch.int32 if fill32 else torch.int64, device="cuda")
        fn = L.rbg_locate_fill_dev32 if fill32 else L.rbg_locate_fill_dev
        rc = fn(*self.args(mh), d_locs.data_ptr(), self.d_ws.data_ptr(), self.st)
        torch.cuda.synchronize()
        if rc:
            return rc, None, None
        assert int(d_locs[total].item()) == -7
        perm = self.d_ws[:4 * N].view(torch.int32).cpu().numpy().astype(np.int64)
        return _u64(self.d_loc_off).copy(), d_locs[:total], perm


def test_locate_on_the_device(case):
    """leg 1: loc_off and the locations equal the oracle's locs_at_batch for every max_hits, without documents, under the small table and under the large
    one, whose 200 documents put the chains in locus order (the permutation changes, the results do not); on A rbg_locate_fill_dev32 gives the low
    words, read as unsigned, with 0xFFFFFFFF for the planted toeholds only; on B and C it is refused"""
    E, rb = case
    ch = _Chain(E, rb)
    perms = {}
    for table in (None, "small", "large"):
        hbm = int(rb.info().hbm_bytes)
        if table:
            _set_docs(E, rb, table)
        for mh in HITS:
            woff, wlocs = E.locs[mh]
            g_off, d_locs, perm = ch.located(mh)
            assert (g_off == woff).all() and (_u64(d_locs) == wlocs).all(), (table, mh)
            assert sorted(perm.tolist()) == list(range(ch.N))
            r32 = ch.located(mh, fill32=True)
            if E.name == "A":
                l32 = r32[1].cpu().numpy().view(np.uint32)
                assert (r32[0] == woff).all() and (l32.astype(np.uint64) == (wlocs & np.uint64(0xFFFFFFFF))).all(), (table, mh)
                assert ((l32 == 0xFFFFFFFF) == (wlocs == np.uint64(MAXU))).all() and int(l32[l32 != 0xFFFFFFFF].max()) >= 2**32 - 2**16
            else:
                assert r32[0] == EARG
        perms[table] = perm
        if table == "large":   # the locus order is active (capi/load.ipp upload_order_docs: its document starts are on the device) and is another order
            assert int(rb.info().hbm_bytes) > hbm and (perm != perms[None]).any()
        elif table == "small":
            assert (perm == perms[None]).all()


def _same(got, want, what):
    for k, w in want.items():
        if got.get(k) is not None:
            assert got[k].shape == w.shape and (got[k] == w).all(), (what, k)


def test_document_hits(case, monkeypatch):
    """leg 2: rbg_doc_hits on the fused path, on the two-step path in one piece and cut into pieces of 100 locations; rbg_doc_hits_dev on the locations
    of leg 1, rbg_doc_hits_dev32 on A, rbg_locate_doc_hits_dev with and without the order; rbg_resolve_offsets_dev -- all against the model over the oracle's
    locations and the oracle's resolve_offset, under both tables"""
    import torch
    E, rb = case
    L = ra.lib()
    ch = _Chain(E, rb)
    N = ch.N
    for table in ("small", "large"):
        names, starts = _set_docs(E, rb, table)
        nd, W = len(starts), (len(starts) + 63) // 64
        # the host call
        for env in ({}, {"RBG_DOC_HITS_FUSED": "0"}, {"RBG_DOC_HITS_FUSED": "0", "RBG_DOC_HITS_CHUNK_LOCS": str(E.chunk_locs)}):
            with monkeypatch.context() as mp:
                mp.delenv("RBG_DOC_HITS_CHUNK", raising=False)
                for k in ("RBG_DOC_HITS_FUSED", "RBG_DOC_HITS_CHUNK_LOCS"):
                    mp.delenv(k, raising=False)
                for k, v in env.items():
                    mp.setenv(k, v)
                res = rb.doc_hits(E.seqs, E.off, 8, doc_locs=True)
            assert (res[0] == E.wlo).all() and (res[1] == E.whi).all()
            _same(dict(zip(("sets", "ndocs", "nodoc", "doc_reads", "doc_locs"), res[2:])), E.docs[table, "host"], (table, env))
        # the device calls, on the stored locations and from the walk itself
        for mh, key in ((8, "dev"), (64, "dev64")):
            want = E.docs[table, key]
            for fill32 in (False, True) if E.name == "A" else (False,):
                g_off, d_locs, _ = ch.located(mh, fill32=fill32)
                d_sets = torch.full((N * W,), -1, dtype=torch.int64, device="cuda")
                d_nd, d_no = (torch.full((N,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
                d_dr = torch.zeros(nd, dtype=torch.int64, device="cuda")
                fn = L.rbg_doc_hits_dev32 if fill32 else L.rbg_doc_hits_dev
                assert fn(rb.h, d_locs.data_ptr(), ch.d_loc_off.data_ptr(), N, d_sets.data_ptr(), d_nd.data_ptr(), d_no.data_ptr(), d_dr.data_ptr(), ch.st) == 0
                torch.cuda.synchronize()
                got = {"sets": _u64(d_sets).reshape(N, W), "ndocs": d_nd.cpu().numpy().view(np.uint32), "nodoc": d_no.cpu().numpy().view(np.uint32), "doc_reads": _u64(d_dr)}
                _same(got, want, (table, mh, "stored locations", fill32))
            for order in (True, False):
                res = rb.locate_doc_hits(ch.d_lo, ch.d_hi, ch.d_k, max_hits=mh, order=order, doc_locs=True)
                torch.cuda.synchronize()
                view = (np.uint64, np.uint32, np.uint32, np.uint64, np.uint64)
                got = {k: r.cpu().numpy().view(v) for k, r, v in zip(("sets", "ndocs", "nodoc", "doc_reads", "doc_locs"), res, view)}
                _same(got, want, (table, mh, "from the walk", order))
        doc, off = rb.resolve_offsets(E.uniq)
        assert (doc == E.resolved[table][0]).all() and (off == E.resolved[table][1]).all(), table


def test_sam(case):
    """leg 3: rbg_align_sam with and without qualities, with and without secondaries, max_hits 1 and 8, and with min_length 1, and rbg_sam_header, under both
    tables: the model's bytes"""
    E, rb = case
    for table in ("small", "large"):
        _set_docs(E, rb, table)
        assert rb.sam_header() == E.header[table]
        for secondary in (False, True):
            for max_hits in (1, 8):
                for ql in (True, False):
                    got = rb.align_sam(E.sam_reads, E.quals if ql else None, E.names, MIN_LENGTH, max_hits, secondary)
                    _same_text(got, E.sam[table, secondary, max_hits, ql], (table, secondary, max_hits, ql))
        _same_text(rb.align_sam(E.sam_reads, None, E.names, 1, 8, True), E.sam[table, "min_length 1"], (table, "min_length 1"))


def _same_text(got, want, what):
    if got == want:
        return
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    m = min(len(a), len(b))
    d = np.nonzero(a[:m] != b[:m])[0]
    at = int(d[0]) if len(d) else m
    raise AssertionError(f"{what}: texts differ at byte {at} (got {len(got)} bytes, want {len(want)}): got {got[max(at - 80, 0):at + 80]!r}, "
                         f"want {want[max(at - 80, 0):at + 80]!r}")


def _lists(res):
    seed_off, cols = res[0], res[1:]
    return [[tuple(int(c[t]) for c in cols) for t in range(int(seed_off[i]), int(seed_off[i + 1]))] for i in range(len(seed_off) - 1)]


def test_seed_lists(case):
    """leg 4: get_seeds_greedy with and without the sample, greedy_longest_seed, find_range_w_toehold_chkpnts and find_locs_greedy_seeding against
    seeds_model and the oracle's greedy_locate"""
    E, rb = case
    seqs, off = ra.pack_reads(E.seed_reads)
    for (ml, ws), want in E.seeds.items():
        got = _lists(rb.get_seeds_greedy(seqs, off, ml, ws))
        for i, q in enumerate(E.seed_reads):
            assert got[i] == want[i], (i, q, ml, ws)
    for ml, want in E.longest.items():
        b = rb.greedy_longest_seed(seqs, off, ml)
        for i in range(len(E.seed_reads)):
            assert tuple(int(a[i]) for a in b) == want[i], (i, ml)
    for wsize, want in E.chk.items():
        got = _lists(rb.find_range_w_toehold_chkpnts(seqs, off, wsize))
        for i, q in enumerate(E.seed_reads):
            assert got[i] == want[i], (i, q, wsize)
    goff, glocs = rb.find_locs_greedy_seeding(seqs, off, MIN_LENGTH, 8)
    assert split(goff, glocs) == E.greedy_locs


def test_markers_at_located_positions(case):
    """leg 5: rbg_markers_at_locs on the locations of leg 1 (the planted 2^64 - 1 among them) and rbg_find_loc_markers_greedy_seeding against the model"""
    E, rb = case
    rb.set_text_markers(*_arrays(E.mk_runs))
    woff, wlocs = E.locs[8]
    mk_off, got = rb.markers_at_locs(wlocs, woff, E.off)
    assert split(mk_off, got) == E.mk_at_locs
    seqs, off = ra.pack_reads(E.seed_reads)
    loc_off, locs, mk_off, got = rb.find_loc_markers_greedy_seeding(seqs, off, MIN_LENGTH, 8)
    assert split(loc_off, locs) == [w[0] for w in E.loc_mk]
    assert split(mk_off, got) == [w[1] for w in E.loc_mk]


def _records(got):
    return [(int(g["ext"]), int(g["nm"]), int(g["score"]), int(g["steps"]), tuple(int(v) for v in g["mis_t"]), tuple(int(v) for v in g["mis_ref"])) for g in got]


def _same_records(got, want, what):
    got = _records(got)
    assert len(got) == len(want), what
    for j, (g, x) in enumerate(zip(got, want)):
        assert g == XM.record_tuple(x), (what, j, g, XM.record_tuple(x))


def test_extension_walks(case, monkeypatch):
    """leg 6: rbg_fl_info and rbg_fl_dev against fl_model, rbg_extend_left_dev against sam_extend_model.extend over the oracle, rbg_extend_right_dev against
    fl_model.extend_right, for every budget; each once with one workgroup striding"""
    E, rb = case
    fl, pb = E.fl, POS_BYTES[E.name]
    rb.fl_prepare()
    info = rb.fl_info()
    assert info["prepared"] and info["bytes"] == fl.bytes(pb) and info["runs"] == [fl.runs(c) for c in b"ACGT"] and info["shift"] == [fl.shift(c) for c in b"ACGT"]
    assert info["dir_entries"] == sum((fl.count[c] >> fl.shift(c)) + 2 for c in b"ACGT")
    left = lambda K: rb.extend_left(E.left["packed"], E.left["off"], E.left["seq"], E.left["pos"], E.left["row"], E.left["limit"], K)
    right = lambda K: rb.extend_right(E.right["packed"], E.right["off"], E.right["seq"], E.right["pos"], E.right["row"], E.right["skip"], E.right["limit"], K)

    def rows():
        gs, gn = rb.fl(E.fl_rows)
        bad = np.flatnonzero((gs != E.fl_sym) | (gn != E.fl_next))
        assert len(bad) == 0, [(int(E.fl_rows[j]), int(gs[j]), int(gn[j]), int(E.fl_sym[j]), int(E.fl_next[j])) for j in bad[:5]]

    rows()
    for K in WALK_KS:
        _same_records(left(K), E.left["want"][K], ("left", K))
        _same_records(right(K), E.right["want"][K], ("right", K))
    monkeypatch.setenv("RBG_SAM_GRID_CAP", "1")
    rows()
    _same_records(left(8), E.left["want"][8], ("left", 8, "one workgroup"))
    _same_records(right(8), E.right["want"][8], ("right", 8, "one workgroup"))
    monkeypatch.delenv("RBG_SAM_GRID_CAP")


def test_sam_extended(case, monkeypatch):
    """leg 7: rbg_align_sam_extend and rbg_align_sam_extend_both under the two tables and the cut one, with and without secondaries, max_hits 1 and 8, budgets
    0, 2 and 4 (qualities at 4): the models' bytes; once with one workgroup striding over the batch three times"""
    E, rb = case
    rb.fl_prepare()
    for table in ("small", "large", "cut"):
        names, starts = E.x_tables[table]
        rb.set_docs(names, starts)
        rb.docs_prepare()
        for K in SAM_KS:
            ql = E.x_quals if K == 4 else None
            for secondary in (False, True):
                for max_hits in (1, 8):
                    for right in (False, True):
                        got = rb.align_sam_extend(E.x_reads, ql, E.x_names, MIN_LENGTH, max_hits, secondary, K, right=right)
                        _same_text(got, E.x_sam[table, right, secondary, max_hits, K], (table, right, secondary, max_hits, K))
        assert E.x_sam[table, True, True, 8, 4] != E.x_sam[table, False, True, 8, 4]
    left = rb.align_sam_extend(E.x_reads, None, E.x_names, MIN_LENGTH, 8, True, 2)
    both = rb.align_sam_extend(E.x_reads, None, E.x_names, MIN_LENGTH, 8, True, 2, right=True)
    assert left != both and len(left.splitlines()) == len(both.splitlines())            # this handle's right walks moved something
    monkeypatch.setenv("RBG_SAM_GRID_CAP", "1")
    _same_text(rb.align_sam_extend(E.x_reads * 3, None, E.x_names * 3, MIN_LENGTH, 8, True, 2, right=True), E.x_sam["cut", True, True, 8, 2] * 3, "one workgroup")
    _same_text(rb.align_sam_extend(E.x_reads * 3, None, E.x_names * 3, MIN_LENGTH, 8, True, 2), E.x_sam["cut", False, True, 8, 2] * 3, "one workgroup, left")
    monkeypatch.delenv("RBG_SAM_GRID_CAP")
