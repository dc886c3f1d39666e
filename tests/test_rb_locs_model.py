"""The rb_locs model (tests/rb_locs_model.py; reference src/rb_markers_tsa.cpp:76-88) on the reference's greedy_seeding fixture with a
hand-written handful of text runs -- the expected text is spelled out --, the three interval rules (a location that wrapped below zero, a
read overhanging the end of the text, an empty read) on one read each, and the .midx file format: written with the .mab writer, read back
with its decoder (CPU only)."""
import os

import numpy as np
import pytest

import orc
import sdsl_writer as W
from rb_locs_model import expected_stdout, loc_markers, markers_at_loc
from synth import SynthIndex

M64 = 2**64 - 1


def mk(seq, pos, allele):
    return pos | (seq << 48) | (allele << 60)


def text_oracle(runs):
    """an Oracle that holds `runs` = [(start, end, [values])] as its marker array: the interval query needs nothing else of it"""
    ot = orc.Oracle.from_runs(np.frombuffer(b"A\x01", np.uint8), np.array([1, 1], np.uint64))
    off = np.cumsum([0] + [len(r[2]) for r in runs]).astype(np.uint64)
    ot.set_markers([r[0] for r in runs], [r[1] for r in runs], off, [v for r in runs for v in r[2]])
    return ot


def test_greedy_seeding_fixture_spelled_out(data_dir):
    """both reads of the fixture locate at text position 10000 and are 36 long: [10000, 10035].  A run ending at 9999 and one starting at
    10036 stay out; a run starting exactly at 10035 is in; values come in run order, unsorted, and repeat from read to read"""
    prefix = os.path.join(data_dir, "greedy_seeding", "ref.fa")
    o = orc.Oracle.load(prefix, orc.SA)
    names, reads = orc.read_fastx(os.path.join(data_dir, "greedy_seeding", "query.fq"))
    assert [len(r) for r in reads] == [36, 36] and [o.greedy_locate(r, 10)[0] for r in reads] == [[10000], [10000]]
    ot = text_oracle([(9000, 9999, [mk(0, 9500, 1)]),
                      (10000, 10004, [mk(0, 10003, 0), mk(0, 10002, 1)]),
                      (10020, 10030, [mk(1, 10025, 2)]),
                      (10035, 10035, [mk(3, 10035, 1)]),
                      (10036, 10050, [mk(0, 10040, 1)])])
    try:
        want = ("1019_good 0/10003/0 0/10002/1 1/10025/2 3/10035/1\n"
                "1019_10 0/10003/0 0/10002/1 1/10025/2 3/10035/1\n")
        assert expected_stdout(o, ot, list(zip(names, reads))) == want
        assert expected_stdout(o, ot, list(zip(names, reads)), wsize=5, max_hits=2) == want
        assert expected_stdout(o, ot, list(zip(names, reads)), max_hits=0) == "1019_good\n1019_10\n"   # no location: the name alone
        assert expected_stdout(o, ot, [(b"short", reads[0][:9])]) == "short\n"                           # no seed of 10 symbols
    finally:
        o.close()
        ot.close()


@pytest.fixture(scope="module")
def idx():
    S = SynthIndex(L=400, H=3, n_sites=8, seed=5)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    yield S, o
    o.close()


def test_location_that_wrapped_below_zero_is_empty(idx):
    """a read that extends text[:30] to the left locates at 0 - 3 in the first haplotype; its end wraps back to 29, below the start: nothing, whatever
    lies at the text's start.  The same stretch in the other two haplotypes (410 apart) locates inside the text and answers as usual."""
    S, o = idx
    ot = text_oracle([(0, 40, [mk(0, 7, 1)]), (405, 409, [mk(1, 408, 0)])])
    try:
        q = b"NNN" + S.text[:30].tobytes()
        locs, got = loc_markers(o, ot, q)
        assert sorted(locs) == [407, 817, M64 - 2] and got == [mk(1, 408, 0)]
        assert markers_at_loc(ot, 0, 30) == [mk(0, 7, 1)]          # (the same stretch located where it lies has them)
        assert markers_at_loc(ot, M64 - 2, 2) == []                # a wrapped location whose end does not wrap back: beyond the text
    finally:
        ot.close()


def test_read_overhanging_the_end_of_the_text(idx):
    """the last 20 symbols before the terminator plus three that match nothing: [n - 21, n + 1] meets the run that ends at n - 1 (the same
    stretch of the two haplotypes before it lies inside the text and meets no run)"""
    S, o = idx
    n = S.n
    ot = text_oracle([(n - 40, n - 30, [mk(0, 1, 0)]), (n - 5, n - 1, [mk(1, 2, 1), mk(1, 3, 0)])])
    try:
        q = S.text[n - 21:n - 1].tobytes() + b"NNN"
        locs, got = loc_markers(o, ot, q)
        assert sorted(locs) == [n - 21 - 820, n - 21 - 410, n - 21] and got == [mk(1, 2, 1), mk(1, 3, 0)]
    finally:
        ot.close()


def test_empty_read_and_zero_length(idx):
    S, o = idx
    ot = text_oracle([(0, S.n - 1, [mk(0, 1, 1)])])
    try:
        assert loc_markers(o, ot, b"") == ([], [])
        assert expected_stdout(o, ot, [(b"empty", b"")]) == "empty\n"
        assert markers_at_loc(ot, 5, 0) == []                 # m == 0: the end lies below the start
        assert markers_at_loc(ot, 0, 0) == [mk(0, 1, 1)]      # ... except at location 0, where l + m - 1 wraps to 2^64 - 1 (no read gets there: an empty read has no location)
        assert markers_at_loc(ot, 5, 1) == [mk(0, 1, 1)]
    finally:
        ot.close()


def test_midx_written_as_mab_decodes_to_its_runs():
    """<prefix>.midx is written with the .mab writer (the equivalence of the two formats is inferred: include/rbg.h)"""
    starts, ends = [0, 40, 80, 4000], [4, 44, 100, 4046]
    off, vals = [0, 1, 3, 4, 7], [mk(0, 2, 1), mk(0, 41, 0), mk(1, 42, 1), mk(2, 90, 3), mk(0, 4001, 0), mk(0, 4002, 1), mk(4095, 4003, 15)]
    data = W.mab_bytes(starts, ends, off, vals, 10, universe=4047)
    u, s, e, f, v, wsize = W.decode_mab(data)
    assert u == 4047 and s.tolist() == starts and e.tolist() == ends and f.tolist() == off and v.tolist() == vals and wsize == 10
