"""The lmem model (tests/lmem_model.py, RowBowt::get_markers_lmems rowbowt.hpp:341-404) against brute force on a synthetic
pangenome: every record's length is the longest suffix of q[:e] that occurs in the text and its range holds that suffix's
occurrences; with an ftab of k-mer size K the hits agree with K = 0 and the misses carry at least K symbols (CPU only)."""
import numpy as np
import pytest

import orc
from lmem_model import lmem_records, LmemAsGreedy
from synth import SynthIndex


@pytest.fixture(scope="module")
def idx():
    S = SynthIndex(L=1500, H=5, n_sites=30, seed=23)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    yield S, o
    o.close()


def _longest_occurring_suffix(fm, p):
    """(length, occurrences) of the longest suffix of p that occurs in the text, by plain binary search on the suffix array"""
    L, cnt = 0, fm.n
    for length in range(1, len(p) + 1):
        lo, hi = fm.find_range(p[len(p) - length:])
        if hi < lo:
            break
        L, cnt = length, hi - lo + 1
    return L, cnt


def _reads(S):
    reads = S.sample_reads(40, 60, seed=7, sub_rate=0.5, ragged=True)
    reads += [b"ACGTTGCAAGGT", b"ACGTN", b"NACGT", b"ACNGTACGTAC", S.text[:90].tobytes(), b"A", b"TTTTTTTTTTTTTTTTTTTTTT"]
    return reads


def test_lengths_and_ranges_match_brute_force(idx):
    S, o = idx
    for q in _reads(S):
        recs = lmem_records(o, q, 10, 2**64 - 1, 0)
        assert len(recs) == len(q)
        for k, (lo, hi, qs, qe, _mk) in enumerate(recs):
            e = len(q) - k
            assert qe == e                                       # end positions m, m-1, ..., 1 in callback order
            L, cnt = _longest_occurring_suffix(S.fm, q[:e])
            assert (qe - qs, hi - lo + 1) == (L, cnt), (q, e)
            if L:
                assert (lo, hi) == S.fm.find_range(q[qs:qe])


@pytest.mark.parametrize("K", [3, 4, 6])
def test_ftab_hits_agree_and_misses_count_k_symbols(idx, K):
    """quirk 1: a miss goes on from the full range with K symbols counted; quirk 3: a suffix shorter than K ignores the ftab"""
    S, o = idx
    misses = 0
    for q in _reads(S):
        plain = lmem_records(o, q, 10, 1000, 0)
        withk = lmem_records(o, q, 10, 1000, K)
        assert len(withk) == len(q)
        for k, (a, b) in enumerate(zip(plain, withk)):
            e = len(q) - k
            if e < K:
                assert a == b, (q, e)                            # quirk 3
                continue
            kmer = q[e - K:e]
            lo, hi = S.fm.find_range(kmer)
            if set(kmer) <= set(b"ACGT") and hi >= lo:
                assert a[:4] == b[:4], (q, e)                    # a hit: the ftab is find_range of the word
            else:
                misses += 1
                assert b[3] - b[2] >= K, (q, e)                  # quirk 1: the K unmatched symbols are part of the seed
    assert misses > 0


def test_failure_at_the_last_symbol_reports_the_full_range(idx):
    """quirk 4: an end position whose symbol does not occur gives the full range and length 0"""
    S, o = idx
    q = b"ACGTACGTN"
    recs = lmem_records(o, q, 4, 1000, 0)
    assert recs[0][:4] == (0, o.n - 1, len(q), len(q))
    assert recs[1][3] == len(q) - 1 and recs[1][2] < recs[1][3]
    recs4 = lmem_records(o, q, 4, 1000, 4)                      # the word ending in N is a miss: K symbols, full range
    assert recs4[0][3] - recs4[0][2] >= 4 and recs4[0][:2] != (1, 0)


def test_empty_sequence_and_markers(idx):
    S, o = idx
    assert lmem_records(o, b"", 10, 1000, 4) == []
    ms, me, mo, mv = S.markers(wsize=10)
    o2 = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    o2.set_markers(ms, me, mo, mv)
    try:
        reads = S.sample_reads(20, 80, seed=9, sub_rate=0.0)
        nmk = sum(len(r[4]) for q in reads for r in lmem_records(o2, q, 10, 1000, 0))
        assert nmk > 0
        # the adapter hands the records to rb_markers_model unchanged
        assert LmemAsGreedy(o2).markers_greedy_seeding(reads[0], 10, 1000, 4) == lmem_records(o2, reads[0], 10, 1000, 4)
        # a max_range of 0 filters every window query
        assert all(not r[4] for r in lmem_records(o2, reads[0], 10, 0, 0))
    finally:
        o2.close()
