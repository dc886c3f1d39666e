"""The seed-list and checkpoint models (tests/seeds_model.py: RowBowt::get_seeds_greedy rowbowt.hpp:191-215,
get_seeds_greedy_w_sample :222-256, find_range_w_toehold_chkpnts :575-606) against what the oracle already answers: every
seed is a fresh search of its own symbols, the longest seed is the oracle's greedy_locate seed and reproduces the reference's
own test values (rb_tests.cpp:83-95), seeds are disjoint and ordered right to left, and the quirk cases (CPU only)."""
import os

import pytest

import golden_values as G
import orc
from seeds_model import MAXU, chkpnt_count, longest_seed, seeds_greedy, toehold_chkpnts
from synth import SynthIndex


@pytest.fixture(scope="module")
def toy(data_dir):
    o = orc.Oracle.load(os.path.join(data_dir, "small.fa"), orc.SA | orc.MA)
    yield o
    o.close()


@pytest.fixture(scope="module")
def idx():
    S = SynthIndex(L=1500, H=5, n_sites=30, seed=23)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    yield S, o
    o.close()


def _toy_reads(data_dir):
    reads = orc.read_fastx(os.path.join(data_dir, "simple_query.fq"))[1] + orc.read_fastx(os.path.join(data_dir, "error_query.fq"))[1]
    return reads + [b"", b"ACG", b"ACGTN", b"N", b"NN", b"acgtacgtac", b"ACGTNNACGT", b"ACGNT"]


def _synth_reads(S):
    reads = S.sample_reads(40, 80, seed=7, sub_rate=0.3, ragged=True)
    return reads + [b"ACGTTGCAAGGT", b"ACGTN", b"NACGT", b"ACNGTACGTAC", S.text[:90].tobytes(), b"A", b""]


def _check_list(o, q, min_length, w_sample):
    recs = seeds_greedy(o, q, min_length, w_sample)
    full = (0, o.n - 1)
    prev_qs = None
    for lo, hi, qs, qe, ss in recs:
        assert qs <= qe <= len(q)
        if qe > qs:                                    # the identity: a seed is a fresh search of q[qs:qe] from the full range
            wlo, whi, wk = o.find_range_w_toehold(q[qs:qe])
            assert (lo, hi) == (wlo, whi) and whi >= wlo, (q, qs, qe)
            assert ss == (wk if w_sample else 0), (q, qs, qe)
            assert qs == 0 or o.find_range(q[qs - 1:qe])[1] < o.find_range(q[qs - 1:qe])[0]   # maximal to the left
        else:
            assert (lo, hi) == full
        if prev_qs is not None:                        # disjoint, right to left, the failing byte between neighbours
            assert qe <= prev_qs - 1
            if min_length == 0:
                assert qe == prev_qs - 1
        prev_qs = qs
    assert all(qe - qs >= min_length for _, _, qs, qe, _ in recs[:-1])
    if recs and (w_sample or min_length == 0):
        assert recs[-1][3] - recs[-1][2] >= min_length
    if min_length == 0 and recs:
        assert recs[0][3] == len(q) and recs[-1][2] == 0
    return recs


@pytest.mark.parametrize("w_sample", [True, False])
def test_seed_identity_and_order(toy, idx, data_dir, w_sample):
    S, o = idx
    nseeds = 0
    for oo, reads in ((toy, _toy_reads(data_dir)), (o, _synth_reads(S))):
        for q in reads:
            for min_length in (0, 1, 5, 10, 21):
                nseeds += len(_check_list(oo, q, min_length, w_sample))
    assert nseeds > 300


def test_longest_seed_is_greedy_locate(toy, idx, data_dir):
    """locate_from_longest_seed on the modelled list == Oracle.greedy_locate, seed and locations"""
    S, o = idx
    for oo, reads in ((toy, _toy_reads(data_dir)), (o, _synth_reads(S))):
        for q in reads:
            for min_length in (1, 10, 21):
                best = longest_seed(seeds_greedy(oo, q, min_length))
                wlocs, (wlo, whi, wqs, wqe, wss) = oo.greedy_locate(q, min_length)
                if best is None:
                    assert wlocs == [] and wqe == wqs
                    continue
                assert best == (wlo, whi, wqs, wqe, wss), (q, min_length)
                assert [(l - best[2]) & MAXU for l in oo.locs_at(best[0], best[1], best[4])] == wlocs


def test_reference_greedy_locate_values(toy, error_reads):
    """rb_tests.cpp:68-95 GreedyLocateTester as the reference wrote it: the list first, locate_from_longest_seed second"""
    assert len(error_reads) == len(G.GREEDY_LOCS_PREFIX)
    for q, want in zip(error_reads, G.GREEDY_LOCS_PREFIX):
        best = longest_seed(seeds_greedy(toy, q, 10))
        locs = [(l - best[2]) & MAXU for l in toy.locs_at(best[0], best[1], best[4])] if best else []
        if want is None:
            assert locs == []
        else:
            assert locs[:len(want)] == want


def test_quirk_cases(toy):
    o = toy
    full = (0, o.n - 1)
    F = full + (0, 0)
    # quirk 5: an empty read
    assert seeds_greedy(o, b"", 0) == [F + (MAXU,)]
    assert seeds_greedy(o, b"", 3) == []
    assert seeds_greedy(o, b"", 0, False) == seeds_greedy(o, b"", 3, False) == [F + (0,)]
    # quirk 6 / 4: N ends a seed and is skipped; zero-length seeds only at min_length 0, pk = 2^64 - 1 before any successful step
    assert seeds_greedy(o, b"N", 0) == [full + (1, 1, MAXU), F + (MAXU,)]
    assert seeds_greedy(o, b"N", 3) == []
    assert seeds_greedy(o, b"N", 3, False) == [F + (0,)]                     # quirk 1: without the sample the tail is always pushed
    assert seeds_greedy(o, b"NN", 0) == [full + (2, 2, MAXU), full + (1, 1, MAXU), F + (MAXU,)]
    q = b"ACGTNNACGT"
    a = seeds_greedy(o, q, 0)
    r_lo, r_hi, r_k = o.find_range_w_toehold(b"ACGT")
    assert r_hi >= r_lo
    # ACGT | N | (empty) | N | ACGT: the zero-length seed between the two N carries the right ACGT's toehold (quirk 4)
    assert a == [(r_lo, r_hi, 6, 10, r_k), full + (5, 5, r_k), (r_lo, r_hi, 0, 4, r_k)]
    assert seeds_greedy(o, q, 3) == [a[0], a[2]]
    assert seeds_greedy(o, q, 5) == []
    assert seeds_greedy(o, q, 5, False) == [(r_lo, r_hi, 0, 4, 0)]
    assert seeds_greedy(o, q, 0, False) == [rec[:4] + (0,) for rec in a]
    assert longest_seed(seeds_greedy(o, b"NN", 0)) is None


def test_no_toehold_sa(data_dir):
    o = orc.Oracle.load(os.path.join(data_dir, "small.fa"), orc.NONE)
    assert seeds_greedy(o, b"ACGTNNACGT", 0) == [] and toehold_chkpnts(o, b"ACGT", 2) == []      # :225, :579
    recs = seeds_greedy(o, b"ACGTNNACGT", 0, False)
    assert [(r[2], r[3], r[4]) for r in recs] == [(6, 10, 0), (5, 5, 0), (0, 4, 0)]
    o.close()


def test_chkpnts_identity_and_counts(toy, idx, error_reads):
    """a checkpoint with qstart = s > 0 is find_range_w_toehold(q[s-1:]) (one symbol ahead of its label), the final one the
    whole read's; the number of records is chkpnt_count(m, wsize)"""
    S, o = idx
    for oo, src in ((toy, error_reads[2]), (o, S.text[200:330].tobytes())):
        for wsize in (1, 3, 5, 10, 19, 20, 64, 300):
            for m in (0, 1, 2, 19, 20, 21, 41, 61, 64, 65, len(src)):
                q = src[max(len(src) - m, 0):] if m else b""
                if m > len(src) or (m and oo.count(q) == 0):
                    continue
                recs = toehold_chkpnts(oo, q, wsize)
                assert len(recs) == chkpnt_count(m, wsize), (wsize, m)
                qe = m
                for lo, hi, qs, qend, ss in recs:
                    if qs > 0:
                        assert (lo, hi, ss) == oo.find_range_w_toehold(q[qs - 1:]) and qend == qe and qe - qs >= wsize
                    elif m:
                        assert (lo, hi, ss) == oo.find_range_w_toehold(q) and qend == m
                    else:
                        assert (lo, hi, qs, qend, ss) == (0, oo.n - 1, 0, 0, oo.last_run_sample())
                    qe = qs
    assert [chkpnt_count(0, w) for w in (1, 2, 3, 5, 7, 15, 17, 19)] == [0, 1, 0, 0, 1, 0, 0, 1]
    assert chkpnt_count(1, 1) == 0 and chkpnt_count(2, 1) == 1 and chkpnt_count(20, 19) == 1 and chkpnt_count(21, 19) == 2


def test_chkpnts_of_a_read_that_does_not_occur(toy, error_reads):
    for q in (b"ACGTN", b"N", error_reads[0] + b"N" + error_reads[0]):
        assert toy.count(q) == 0
        assert toehold_chkpnts(toy, q, 3) == []
