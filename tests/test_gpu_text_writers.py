"""GPU parity of the two kernels that write the tools' text -- k_text_write (k_text.hip: rbg_align_text, `rb_align -s [-m]`) and k_report_write
(k_report.hip: rbg_markers_report_text, `rb_markers --device-format`) -- where the other GPU files leave them untested: decimals of every width
at the powers of ten, a workgroup's 256 elements at exactly the bytes it stages in LDS and one byte more, every alignment (mod 16) of a staged
block's first byte, grids at their caps, the -m markers line across blocks and beyond the staging limit, document tables at their edges.

The reference of every case is text built here with Python integers (on top of orc.Oracle's locs_at / resolve_offset / markers_at, and
rb_markers_model.expected_stdout for the report); every comparison is of the whole output, byte for byte.  A case built to reach a branch asserts
from the EXPECTED text that it does: the bytes of elements 256 b .. 256 b + 255 are summed and compared with the limit, which is read from the
kernel's source (kTextLds, kReportLds, the grid caps), so that a change of the constant fails the test instead of moving it off the boundary.
The text is written to a fresh device allocation (256-byte aligned), so a block's first byte has the alignment of its offset in the text.

Left out: the grid caps of the report's kernels.  They need 10^6 elements, which real seeding does not produce within a test's seconds, and
there is no entry point that takes records directly."""
import os
import re
import shutil

import numpy as np
import pytest

import golden_values as G
import orc
import rb_markers_model as RM
import rowbowt_amd as ra
from rowbowt_amd import capi
from gpu_common import _run_cli, _random_run_index, _lf_walk_reads, _with_layout
from synth import SynthIndex

pytestmark = pytest.mark.gpu
M64 = 2**64 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_MARKERS = b"no markers (consider building the marker array with a larger window size)"
EARG = -4


def _source(fname):
    with open(os.path.join(ROOT, "rowbowt_amd", "csrc", fname)) as f:
        return f.read()


def _lds_limit(fname, name):
    """bytes of text a workgroup stages, from the kernel's source"""
    m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*\*\s*1024\s*;" % name, _source(fname))
    assert m, f"{name} = <k> * 1024 not found in {fname}: this file's boundary cases follow that constant"
    return int(m.group(1)) * 1024


def _text_grid_caps():
    """the most workgroups k_text_mark, k_text_len and k_text_write are launched with (each takes 256 elements per turn)"""
    caps = [int(a) * int(b) for a, b in re.findall(r"\+ 255\) / 256, (\d+)ull \* (\d+)\)", _source("k_text.hip"))]
    assert len(caps) == 3, f"the three grid caps of k_text.hip were not found: {caps}"
    return caps


def _same(got, want):
    """whole-output equality; on a mismatch, the first differing byte and what surrounds it"""
    if got == want:
        return
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    m = min(len(a), len(b))
    at = m
    for s in range(0, m, 1 << 20):
        d = np.nonzero(a[s:s + (1 << 20)] != b[s:s + (1 << 20)])[0]
        if len(d):
            at = s + int(d[0])
            break
    raise AssertionError(f"texts differ at byte {at} (got {len(got)} bytes, want {len(want)}): got {got[max(at - 60, 0):at + 60]!r}, "
                         f"want {want[max(at - 60, 0):at + 60]!r}")


def _block_bytes(elems):
    """the bytes of every workgroup's 256 elements"""
    return [sum(len(e) for e in elems[b:b + 256]) for b in range(0, len(elems), 256)]


def _letters(rng, n):
    return bytes(rng.integers(ord("a"), ord("z") + 1, n, dtype=np.uint8))


def _resolve(o, l):
    """the oracle's resolve_offset -> (name bytes or None, offset); None: no document starts at or before l"""
    off = orc.U64()
    name = o.L.orc_resolve_offset(o.h, l, off)
    return name, off.value


def _text_elems(o, names, lo, hi, k=None, max_hits=M64, markers=False):
    """rb_report's text (rb_align.cpp:118-145) as the list of k_text.hip's elements: per read the head, one element per location (the last carries
    the newline), the markers line.  None if a location lies before every document (the reference reads doc_names_[-1] there; the library says
    RBG_EARG)."""
    if k is not None:
        loc_off, locs = o.locs_at_batch(np.ascontiguousarray(lo, dtype=np.uint64), np.ascontiguousarray(hi, dtype=np.uint64),
                                        np.ascontiguousarray(k, dtype=np.uint64), max_hits)
        loc_off, locs = loc_off.tolist(), locs.tolist()
        res = {l: _resolve(o, l) for l in set(locs)}
    elems = []
    for i, n in enumerate(names):
        a, b = int(lo[i]), int(hi[i])
        head = b"%s (%d,%d), count=%d\n" % (n, a, b, (b - a + 1) & M64)
        if k is None:
            elems.append(head)
        else:
            mine = locs[loc_off[i]:loc_off[i + 1]]
            elems.append(head + b"\tlocs: " + (b"" if mine else b"\n"))
            for j, l in enumerate(mine):
                dn, offs = res[l]
                if dn is None:
                    return None
                elems.append(b"%d/%s:%d " % (l, dn, offs) + (b"\n" if j + 1 == len(mine) else b""))
        if markers:
            mk = o.markers_at(a, b) if a <= b else []
            elems.append(b"\tmarkers: " + (b"".join(b"%d/%d " % (G.get_pos(m), G.get_allele(m)) for m in mk) if mk else NO_MARKERS) + b"\n")
    return elems


def _padded(base, targets, rng):
    """names of letters such that the 256-element block b of `base` (the elements' lengths with empty names, one element per name) has
    targets[b] bytes"""
    names = []
    for b, t in enumerate(targets):
        blk = base[256 * b:256 * (b + 1)]
        need = t - sum(blk)
        assert blk and need >= 0
        q, r = divmod(need, len(blk))
        names += [_letters(rng, q + (1 if j < r else 0)) for j in range(len(blk))]
    assert len(names) == len(base)
    return names


# ---- a. count-only lines: any 64-bit range ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def synth_pair(synth):
    rb = ra.RowBowt.from_runs(synth.heads, synth.lens, synth.ssa, synth.esa, device=0)
    o = orc.Oracle.from_runs(synth.heads, synth.lens, synth.ssa, synth.esa)
    yield synth, rb, o
    rb.close()
    o.close()


def test_count_lines_every_digit_width(synth_pair):
    """lo, hi and count= of 1 to 20 digits, on both sides of every power of ten; hi = 2^64 - 1; empty ranges whose count wraps to 19 and 20
    digits; (0, 2^64 - 1), whose count wraps to 0; names of 0, 1, 15, 16 and 17 bytes"""
    _, rb, _ = synth_pair
    pairs = []
    for k in range(20):
        edge = (10**k - 1, 10**k)
        pairs += [(a, b) for a in edge for b in edge]
        pairs += [(0, 10**k - 1), (1, 10**k - 1), (10**k, M64), (10**k - 1, M64)]       # count = 10^k, 10^k - 1, 2^64 - 10^k, ...
        if k:
            pairs += [(10**k, 10**k - 2), (10**k + 1, 10**k - 1)]                       # hi < lo - 1: count = 2^64 - 1
    pairs += [(10**19, 5), (M64, 10**18), (M64, M64), (M64, 0), (0, M64), (0, 0), (1, 0), (2, 0)]
    lo, hi = [p[0] for p in pairs], [p[1] for p in pairs]
    count = [(b - a + 1) & M64 for a, b in pairs]
    for vals in (lo, hi, count):
        assert {len(str(v)) for v in vals} == set(range(1, 21))
    assert 0 in count and M64 in count and any(len(str(c)) == 19 and b < a - 1 for (a, b), c in zip(pairs, count))
    rng = np.random.default_rng(5)
    names = [_letters(rng, (0, 1, 15, 16, 17)[(i + i // 5) % 5]) for i in range(len(pairs))]
    assert {len(n) for n in names} == {0, 1, 15, 16, 17}
    got = rb.align_text(np.array(lo, dtype=np.uint64), np.array(hi, dtype=np.uint64), None, names)
    _same(got, b"".join(_text_elems(None, names, lo, hi)))


def test_count_lines_at_the_staging_limit(synth_pair):
    """k_text_write's two paths and the copy-out of the staged one: a block of exactly kTextLds bytes (staged), the next of kTextLds + 1
    (every lane writes its element to memory), a short one; the same behind a leading block of s more than a multiple of 16 bytes for
    s = 0..15, which is the alignment of the staged block's first byte (head bytes, 16-byte body, tail); a last block that is partial and
    over the limit; one name of 50 000 bytes in an otherwise short block"""
    _, rb, _ = synth_pair
    limit = _lds_limit("k_text.hip", "kTextLds")
    rng = np.random.default_rng(6)

    def batch(n):
        lo = rng.integers(0, 10**5, n).tolist()
        hi = [a + int(d) for a, d in zip(lo, rng.integers(0, 50, n))]
        return lo, hi, [len(e) for e in _text_elems(None, [b""] * n, lo, hi)]

    def run(lo, hi, names):
        elems = _text_elems(None, names, lo, hi)
        _same(rb.align_text(np.array(lo, dtype=np.uint64), np.array(hi, dtype=np.uint64), None, names), b"".join(elems))
        return _block_bytes(elems)

    lo, hi, base = batch(768)
    assert run(lo, hi, _padded(base, [limit, limit + 1, 9000], rng)) == [limit, limit + 1, 9000]
    shifts = set()
    for s in range(16):
        lo, hi, base = batch(1024)
        lead = 9000 + (s - 9000) % 16
        got = run(lo, hi, _padded(base, [lead, limit, limit + 1, 9000], rng))
        assert got == [lead, limit, limit + 1, 9000] and lead % 16 == s
        shifts.add(got[0] % 16)                                  # where the staged block of exactly `limit` bytes starts
    assert shifts == set(range(16))
    lo, hi, base = batch(256 + 100)                              # E no multiple of 256, the partial block unstaged
    assert run(lo, hi, _padded(base, [9000, limit + 77], rng)) == [9000, limit + 77]
    lo, hi, base = batch(600)
    names = [_letters(rng, 1 + i % 9) for i in range(600)]
    names[300] = _letters(rng, 50000)
    sums = run(lo, hi, names)
    assert len(sums) == 3 and sums[0] < limit // 4 and sums[1] > limit and sums[2] < limit // 4


def test_count_lines_beyond_the_grid_caps(synth_pair):
    """one call of N = 256 * 256 * 32 + 300 reads: more 256-element turns than k_text_mark / k_text_len (cap 256 * 32 workgroups) and k_text_write
    (256 * 16) have workgroups, so every grid-stride loop goes round again, k_text_write's three times over"""
    _, rb, _ = synth_pair
    caps = _text_grid_caps()
    n = 256 * 256 * 32 + 300
    assert sorted(caps) == [256 * 16, 256 * 32, 256 * 32] and n > 256 * max(caps) and n > 2 * 256 * min(caps) and n % 256
    rng = np.random.default_rng(7)
    lo = rng.integers(0, 1 << 40, n, dtype=np.uint64) >> rng.integers(0, 40, n).astype(np.uint64)
    hi = lo + rng.integers(0, 5000, n).astype(np.uint64) - np.uint64(1)                       # (some empty: count=0; lo = 0 wraps hi)
    pool = [_letters(rng, 1 + j % 9) for j in range(63)]
    names = [pool[(i + i // 256) % 63] for i in range(n)]
    assert {len(x) for x in names[:64]} == set(range(1, 10))
    got = rb.align_text(lo, hi, None, names)
    want = b"".join([b"%s (%d,%d), count=%d\n" % (x, a, b, (b - a + 1) & M64) for x, a, b in zip(names, lo.tolist(), hi.tolist())])
    _same(got, want)


# ---- b. locations and documents ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def loc_case(synth_pair):
    """about 2 000 reads of the synthetic pangenome with the oracle's (lo, hi, k): some 20 000 elements, 80 workgroups' worth"""
    S, rb, o = synth_pair
    reads = [q for q in S.sample_reads(2700, 40, seed=41, sub_rate=0.15, ragged=True) if len(q) >= 10][:2000]
    lo, hi, k = o.find_range_w_toehold_batch(*ra.pack_reads(reads))
    names = [b"r%d" % i for i in range(len(reads))]
    _, locs = o.locs_at_batch(lo, hi, k)
    return S, rb, o, names, lo, hi, k, locs


def _docs_case(case, dnames, starts, max_hits=M64, host_too=False):
    S, rb, o, names, lo, hi, k, locs = case
    rb.set_docs(dnames, starts)
    o.set_docs(dnames, starts)
    elems = _text_elems(o, names, lo, hi, k, max_hits)
    assert elems is not None and len(elems) >= len(names) and (max_hits < 3 or len(elems) > 8 * 256)
    _same(rb.align_text(lo, hi, k, names, max_hits), b"".join(elems))
    if host_too:   # the host's rbg_resolve_offset answers like the oracle as well (and so like the device)
        for l in np.unique(locs)[::7].tolist():
            dn, offs = _resolve(o, l)
            assert rb.resolve_offset(l) == (dn.decode(), offs), l
    return elems


def test_documents_at_their_edges(loc_case):
    """doc_of and the offsets on one handle whose table is replaced between calls (the device copy follows): locations equal to a document's
    start and to a start - 1, in the last document, before the second start; names of 0, 1 and 300 bytes; max_hits 2^64 - 1, 2 and 0; one
    document; 5 000 documents; a name of 50 000 bytes, whose locations push their blocks past the staging limit; a first document that starts
    behind a location (RBG_EARG, and the next call with a valid table is right)"""
    S, rb, o, names, lo, hi, k, locs = loc_case
    limit = _lds_limit("k_text.hip", "kTextLds")
    U = np.unique(locs).tolist()
    seen = set(U)
    q = len(U) // 5
    starts = sorted({0, U[q], U[2 * q] + 1, U[3 * q], U[3 * q] + 1, U[4 * q]})
    assert any(s in seen for s in starts[1:]) and any(s - 1 in seen for s in starts[1:]) and U[-1] >= starts[-1] and U[0] < starts[1]
    dnames = ["", "a", "x" * 300] + [f"doc{j}" for j in range(3, len(starts))]
    for max_hits in (M64, 2, 0):
        _docs_case(loc_case, dnames, starts, max_hits)
    _docs_case(loc_case, ["only"], [0])
    rng = np.random.default_rng(8)
    many = [0] + sorted(rng.choice(np.arange(1, S.n), 4999, replace=False).tolist())
    elems = _docs_case(loc_case, [f"d{j}" for j in range(5000)], many)
    assert len({e.split(b"/")[1].split(b":")[0] for e in elems if b"/" in e}) > 2000          # thousands of the documents are printed
    # a document of some tens of locations with a name of 50 000 bytes
    j, w = len(U) // 2, 10
    a, b = U[j], U[j + w]
    inside = int(((locs >= a) & (locs < b)).sum())
    assert 5 <= inside <= 400
    sums = _block_bytes(_docs_case(loc_case, ["p", "L" * 50000, "q"], [0, a, b]))
    assert max(sums) > limit and min(sums) <= limit and sum(sums) > inside * 50000
    # RBG_EARG, then a valid table on the same handle
    bad = [U[0] + 1, U[len(U) // 2]]
    rb.set_docs(["late", "z"], bad)
    o.set_docs(["late", "z"], bad)
    assert _text_elems(o, names, lo, hi, k) is None
    with pytest.raises(ra.RbgError) as ei:
        rb.align_text(lo, hi, k, names)
    assert ei.value.code == EARG
    _docs_case(loc_case, dnames, starts)


def test_documents_given_out_of_order(loc_case):
    """a table whose starts are not ascending: the reference sorts the starts but not the names, and takes the collection's size from the LAST
    start given (doclist.hpp:57-79); whatever the oracle's resolve_offset says of such a table is what the device prints -- with the last start
    given 0 (size 1: every location resolves against the first sorted start), in the middle, and 5 000 starts shuffled"""
    S, rb, o, names, lo, hi, k, locs = loc_case
    U = np.unique(locs).tolist()
    q = len(U) // 5
    starts = sorted({0, U[q], U[2 * q] + 1, U[3 * q], U[4 * q]})
    dnames = [f"n{j}" for j in range(len(starts))]
    _docs_case(loc_case, dnames, starts[::-1], host_too=True)                                  # last given: 0
    _docs_case(loc_case, dnames, starts[2:] + starts[:2], host_too=True)                        # last given: the second smallest
    _docs_case(loc_case, dnames, [starts[-1]] + starts[:-1], host_too=True)                     # last given: the second largest
    rng = np.random.default_rng(9)
    many = np.array([0] + sorted(rng.choice(np.arange(1, S.n), 4999, replace=False).tolist()))
    perm = rng.permutation(5000)
    assert many[perm][-1] not in (0, int(many.max()))
    _docs_case(loc_case, [f"d{j}" for j in range(5000)], many[perm].tolist(), host_too=True)


def test_positions_of_ten_to_twelve_digits():
    """a run list of n between 2^38 and 2^40 (2 000 runs of up to 5 * 10^8 rows; samples are distinct random values below n): locations, document
    starts and offsets of 10 to 12 digits through k_text_len / put_element"""
    rng = np.random.default_rng(4343)
    heads, lens, ssa, esa, n = _random_run_index(rng, 2000, 500_000_000)
    assert (1 << 38) < n < (1 << 40)
    o = orc.Oracle.from_runs(heads, lens, ssa, esa)
    reads = _lf_walk_reads(o, heads, lens, n, rng, 700, 40)
    lo, hi, k = o.find_range_w_toehold_batch(*ra.pack_reads(reads))
    with capi.default_option(capi.OPT_KMER_STEPS, 1):
        rb = _with_layout(capi.LAYOUT_RUNS, lambda: ra.RowBowt.from_runs(heads, lens, ssa, esa, device=0))
    starts = [0, 2_000_000_000, 300_000_000_000]
    assert [len(str(s)) for s in starts] == [1, 10, 12] and starts[-1] < n
    dnames = ["a", "chr10", "z" * 20]
    rb.set_docs(dnames, starts)
    o.set_docs(dnames, starts)
    names = [b"w%d" % i for i in range(len(reads))]
    elems = _text_elems(o, names, lo, hi, k, 8)
    assert elems is not None and len(elems) > 8 * 256
    shown = [e.split(b"/")[0] for e in elems if b"/" in e]
    assert {10, 11, 12} <= {len(p) for p in shown} and all(any(b"/" + d.encode() + b":" in e for e in elems) for d in dnames)
    assert {len(str(int(v))) for v in lo} >= {10, 11, 12}
    _same(rb.align_text(lo, hi, k, names, 8), b"".join(elems))
    rb.close()
    o.close()


# ---- c. the -m markers line --------------------------------------------------------------------------------------------------------------

def _wide_positions(rng, count):
    """marker positions of 1 to 15 digits, each width alike often (below 2^48)"""
    w = rng.integers(1, 16, count)
    lows = np.array([0, 0] + [10**(x - 1) for x in range(2, 16)], dtype=np.uint64)
    highs = np.array([1] + [min(10**x, 1 << 48) for x in range(1, 16)], dtype=np.uint64)
    span = (highs[w] - lows[w]).astype(np.float64)
    return np.minimum(lows[w] + (rng.random(count) * span).astype(np.uint64), highs[w] - np.uint64(1))


def test_markers_line_across_blocks():
    """rb_align -s -m's third line (per_read == 2 in k_text.hip) for 1 500 reads, with and without the locations: heads, locations and markers
    lines interleave over many workgroups; rows carry from 0 to 6 000 markers of positions of 1 to 15 digits (up to 2^48 - 1) and alleles 0, 9, 10
    and 15, the sequence bits set at random (not printed); reads without a match, with a match and no marker, with one marker, and reads whose
    markers line alone is longer than what a workgroup stages"""
    limit = _lds_limit("k_text.hip", "kTextLds")
    rng = np.random.default_rng(10)
    S = SynthIndex(L=1500, H=5, n_sites=30, seed=23)
    rb = ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    reads = S.sample_reads(1500, 40, seed=9, sub_rate=0.1)
    lo, hi, k = o.find_range_w_toehold_batch(*ra.pack_reads(reads))
    nruns = S.n // 3
    starts = np.arange(nruns, dtype=np.uint64) * np.uint64(3)
    ends = starts + np.uint64(2)
    per = rng.choice([0, 0, 0, 1, 1, 2, 5], nruns)
    matched = np.nonzero(hi >= lo)[0]
    heavy = [min(int(lo[matched[len(matched) // 3]]) // 3, nruns - 1), min(int(lo[matched[2 * len(matched) // 3]]) // 3, nruns - 1)]
    per[heavy[0]], per[heavy[1]] = 6000, 5000
    off = np.concatenate(([0], np.cumsum(per))).astype(np.uint64)
    total = int(off[-1])
    pos = _wide_positions(rng, total)
    pos[int(off[heavy[0]])] = (1 << 48) - 1
    vals = (pos | (rng.integers(0, 4096, total).astype(np.uint64) << np.uint64(48))
            | (rng.choice(np.array([0, 9, 10, 15], dtype=np.uint64), total) << np.uint64(60)))
    rb.set_markers(starts, ends, off, vals)
    o.set_markers(starts, ends, off, vals)
    rb.set_docs(S.doc_names, S.doc_starts)
    o.set_docs(S.doc_names, S.doc_starts)
    names = [b"m%d" % i for i in range(len(reads))]
    for with_locs in (True, False):
        elems = _text_elems(o, names, lo, hi, k if with_locs else None, markers=True)
        lines = [e for e in elems if e.startswith(b"\tmarkers: ")]
        nmark = [e.count(b"/") for e in lines]
        assert len(lines) == len(reads) and len(elems) > (12 if with_locs else 8) * 256
        assert max(len(e) for e in lines) > limit and max(nmark) >= 5000 and 1 in nmark                 # over the limit by itself; one marker
        none = [i for i, e in enumerate(lines) if e == b"\tmarkers: " + NO_MARKERS + b"\n"]
        assert any(hi[i] < lo[i] for i in none) and any(hi[i] >= lo[i] for i in none)                   # no match; a match without markers
        printed = b"".join(lines)
        assert {len(p) for p in re.findall(rb"(\d+)/\d+ ", printed)} == set(range(1, 16)) and b" 281474976710655/" in printed
        assert set(re.findall(rb"/(\d+) ", printed)) == {b"0", b"9", b"10", b"15"}
        sums = _block_bytes(elems)
        assert max(sums) > limit and sum(1 for s in sums if s <= limit) > 6
        _same(rb.align_text(lo, hi, k if with_locs else None, names, markers=True), b"".join(elems))
    rb.close()
    o.close()


# ---- d. the report writer ----------------------------------------------------------------------------------------------------------------

def _report_text(rb, recs, **kw):
    seqs, off = ra.pack_reads([s for _, s in recs])
    return rb.markers_report_text(seqs, off, [n for n, _ in recs], capi.report_params(**kw))


def test_report_lines_at_the_staging_limit():
    """k_report_write's two paths on an index without markers, where every record is one element ("<name> <range> <strand> <start> <len> .\\n"):
    a block of 256 records of exactly kReportLds bytes, the next of kReportLds + 1, a short one, behind a leading block of s more than a multiple
    of 16 bytes for s = 0..15.  Reads print two to eight records each; reads are laid out so that none straddles two blocks, and the names
    are padded until the block totals -- taken from the model's text -- hold"""
    limit = _lds_limit("k_report.hip", "kReportLds")
    rng = np.random.default_rng(12)
    S = SynthIndex(L=1500, H=5, n_sites=30, seed=23)
    rb = ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    pool = [b"ACNNGT", b"", b"C", b"ACGT", b"NNNNNN"] + S.sample_reads(400, 30, seed=7, sub_rate=0.3)
    nrec = [RM.expected_stdout(o, [(b"", q)], wsize=4).count("\n") for q in pool]
    count = dict(zip(pool, nrec))
    assert 2 in nrec and 3 in nrec and max(nrec) > 5
    two, three = pool[nrec.index(2)], pool[nrec.index(3)]
    # four blocks of exactly 256 records each, no read across a block's end: a read of two records and one of three (their names take what does
    # not divide among the others), the pool in order, then reads of two and three records up to 256
    seqs, blocks, t = [], [], 0
    for _ in range(4):
        mine, fill = [two, three], 5
        while 256 - fill >= 2 + max(nrec):
            q = pool[t % len(pool)]
            t += 1
            mine.append(q)
            fill += count[q]
        rem = 256 - fill
        mine += [three] * (rem % 2) + [two] * ((rem - 3 * (rem % 2)) // 2)
        assert sum(count[q] for q in mine) == 256
        blocks.append(list(range(len(seqs), len(seqs) + len(mine))))
        seqs += mine
    base = _block_bytes(RM.expected_stdout(o, [(b"", q) for q in seqs], wsize=4).encode().splitlines(keepends=True))
    shifts = set()
    for s in range(16):
        lead = 9000 + (s - 9000) % 16
        lens = [0] * len(seqs)
        for b, target in enumerate([lead, limit, limit + 1, 8000]):
            need = target - base[b]
            share = need // 256 - 1
            rest = need - 256 * share                            # 256 .. 511 bytes left: 2 x + 3 y with y = 0 or 1
            assert share >= 0
            for i in blocks[b]:
                lens[i] = share
            lens[blocks[b][0]] += (rest - 3 * (rest % 2)) // 2
            lens[blocks[b][1]] += rest % 2
        recs = [(_letters(rng, n), q) for n, q in zip(lens, seqs)]
        want = RM.expected_stdout(o, recs, wsize=4).encode()
        lines = want.splitlines(keepends=True)
        assert all(line.endswith(b" .\n") for line in lines)     # one element per record
        sums = _block_bytes(lines)
        assert sums == [lead, limit, limit + 1, 8000] and lead % 16 == s
        shifts.add(sums[0] % 16)
        _same(_report_text(rb, recs, wsize=4), want)
    assert shifts == set(range(16))
    rb.close()
    o.close()


def test_report_marker_triples_of_every_width():
    """" <seq>/<pos>/<allele>" elements with sequence ids 0, 9, 10, 999 and 4095, positions of 1 to 15 digits (up to 2^48 - 1) and alleles 0 to 15,
    on the many-markers-per-row index of test_report_dense_markers"""
    rng = np.random.default_rng(19)
    S = SynthIndex(L=1500, H=5, n_sites=30, seed=23)
    rb = ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    nruns = S.n // 3
    starts = np.arange(nruns, dtype=np.uint64) * np.uint64(3)
    ends = starts + np.uint64(2)
    off = np.concatenate(([0], np.cumsum(rng.integers(0, 25, nruns)))).astype(np.uint64)
    total = int(off[-1])
    pos = _wide_positions(rng, total)
    pos[::97] = (1 << 48) - 1
    vals = (pos | (rng.choice(np.array([0, 9, 10, 999, 4095], dtype=np.uint64), total) << np.uint64(48))
            | (rng.integers(0, 16, total).astype(np.uint64) << np.uint64(60)))
    rb.set_markers(starts, ends, off, vals)
    o.set_markers(starts, ends, off, vals)
    recs = [(b"d%d" % i, q) for i, q in enumerate(S.sample_reads(4, 40, seed=5, sub_rate=0.1) + [b"ACGTTGCA", b"C"])]
    for kw in (dict(wsize=1, max_range=M64), dict(wsize=3, max_range=40)):
        want = RM.expected_stdout(o, recs, **kw).encode()
        triples = re.findall(rb" (\d+)/(\d+)/(\d+)", want)
        assert len(triples) > 2000
        assert {t[0] for t in triples} == {b"0", b"9", b"10", b"999", b"4095"} and {int(t[2]) for t in triples} == set(range(16))
        assert {len(t[1]) for t in triples} == set(range(1, 16)) and any(t[1] == b"281474976710655" for t in triples)
        _same(_report_text(rb, recs, **kw), want)
    rb.close()
    o.close()


# ---- e. through rb_align -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("markers", [False, True], ids=["s", "s-m"])
def test_cli_blocks_beyond_the_staging_limit(data_dir, tmp_path, small, simple_reads, error_reads, markers):
    """`rb_align -s` and `rb_align -s -m` on 300 reads of which one has a name of 45 000 bytes: in every batching (one batch, --batch 100 which
    divides the input, --batch 64 which does not) some workgroup's block goes past the staging limit and others do not; the bytes are the oracle's
    rendering and the host formatter's (RB_ALIGN_HOST_TEXT=1)"""
    limit = _lds_limit("k_text.hip", "kTextLds")
    _, o = small
    for suf in (".rbwt", ".tsa", ".mab"):
        shutil.copy(os.path.join(data_dir, "small.fa" + suf), tmp_path / ("idx" + suf))
    (tmp_path / "idx.docs").write_text("ref 0\nhap1 10010\nhap2 20020\n")
    o.set_docs(["ref", "hap1", "hap2"], [0, 10010, 20020])
    kinds = list(simple_reads) + list(error_reads) + [b"ACGT", simple_reads[0][:30]]
    ranges = [o.find_range_w_toehold(q) for q in kinds]
    N = 300
    reads = [kinds[i % len(kinds)] for i in range(N)]
    lo, hi, k = (np.array([ranges[i % len(kinds)][j] for i in range(N)], dtype=np.uint64) for j in range(3))
    names = [b"c%d" % i for i in range(N)]
    names[20], names[157] = b"m" * 900, b"L" * 45000
    fq = tmp_path / "q.fq"
    fq.write_bytes(b"".join(b"@%s desc %d\n%s\n+\n%s\n" % (n, i, q, b"~" * len(q)) for i, (n, q) in enumerate(zip(names, reads))))
    want = b"".join(_text_elems(o, names, lo, hi, k, markers=markers)).decode()
    flags = ["-s", "-m"] if markers else ["-s"]
    for batch in (N, 100, 64):
        sums = []
        for b0 in range(0, N, batch):
            sl = slice(b0, b0 + batch)
            sums += _block_bytes(_text_elems(o, names[sl], lo[sl], hi[sl], k[sl], markers=markers))
        assert max(sums) > limit and sum(1 for s in sums if s <= limit) >= 2, (batch, sums)
        if batch == (100 if markers else N):
            continue                                            # (three runs of the tool per case: each mode runs two of the batchings)
        rc, out, err = _run_cli(flags + (["--batch", str(batch)] if batch != N else []) + [str(tmp_path / "idx"), str(fq)])
        assert rc == 0, err
        _same(out.encode(), want.encode())
    rc, out, err = _run_cli(flags + [str(tmp_path / "idx"), str(fq)], env={"RB_ALIGN_HOST_TEXT": "1"})
    assert rc == 0, err
    _same(out.encode(), want.encode())
