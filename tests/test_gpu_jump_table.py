"""GPU parity of the jump table (RBG_OPT_JUMP_K; rbg_jump.h, k_jump.hip): a staged read of at least K symbols replaces its first K
backward-search steps by one probe of the table of the K-mers that occur.  Bit-exact lo / hi / toehold, counts and locations against
the oracle on hits, absent keys, lengths around K, symbols outside ACGT in the last K, toeholds that wrap below zero; the layout is the
one the load makes without the table; a replica answers identically.  The probe lives in the STAGED byte-form walk of k_find_range_runs, so
every query here goes there: the host path with 2-bit packing off (OPT_PACKED_READS = 0; it packs batches of 4096 reads or more by
default) and the *_dev entry points; the instrumented search (rbg_find_range_stats_dev) shows that the probe answered."""
import os

import numpy as np
import pytest

import orc
import rowbowt_amd as ra
from rowbowt_amd import capi
from gpu_common import _with_layout

pytestmark = pytest.mark.gpu
MAXU = 2**64 - 1
ST_STEPS, ST_FTAB, ST_SYMBOLS = 0, 4, 7      # rbg_dev.h kStSteps, kStFtab (ftab entries + probed buckets), kStSymbols


@pytest.fixture(autouse=True)
def _byte_form():
    """the host path hands every batch to the byte kernel (which stages the reads) instead of packing large ones"""
    with capi.default_option(capi.OPT_PACKED_READS, 0):
        yield


def _dev_search(rb, seqs, off, toehold):
    """rbg_find_range_stats_dev on device arrays: (lo, hi, k or None, the instrumented sums)"""
    import torch
    N = len(off) - 1
    dev = torch.device("cuda:0")
    d_seqs = torch.from_numpy(np.concatenate([seqs, np.zeros((-len(seqs)) % 16 + 16, np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_lo, d_hi, d_k = (torch.empty(max(N, 1), dtype=torch.int64, device=dev) for _ in range(3))
    d_st = torch.zeros(16, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    rc = ra.lib().rbg_find_range_stats_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, d_lo.data_ptr(), d_hi.data_ptr(),
                                          d_k.data_ptr() if toehold else None, d_st.data_ptr(), st)
    assert rc == 0
    torch.cuda.synchronize()
    u = lambda t: t.cpu().numpy().view(np.uint64)[:N]
    return u(d_lo), u(d_hi), (u(d_k) if toehold else None), d_st.cpu().numpy().tolist()


def _load(S, jump_k, pos_bytes=0):
    ra.set_default_option(capi.OPT_POS_BYTES, pos_bytes)
    try:
        with capi.default_option(capi.OPT_JUMP_K, jump_k):
            return _with_layout(capi.LAYOUT_RUNS, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    finally:
        ra.set_default_option(capi.OPT_POS_BYTES, 0)


def _reads(S, K):
    rng = np.random.default_rng(K)
    text = S.text.tobytes()
    reads = S.sample_reads(2000, 100, seed=K, sub_rate=0.0)                # hits
    reads += S.sample_reads(1000, 100, seed=K + 1, sub_rate=0.5)           # many with a substitution in the last K: absent keys
    for m in (K - 1, K, K + 1):                                            # lengths around K, hits and misses
        reads += S.sample_reads(300, m, seed=K + m, sub_rate=0.0)
        reads += S.sample_reads(300, m, seed=K + m + 7, sub_rate=0.3)
    reads += S.sample_reads(500, 2 * K + 20, seed=K + 3, sub_rate=0.0, ragged=True)
    # a symbol outside ACGT inside the last K (the wave then walks bytes) and one before it
    base = S.sample_reads(200, 100, seed=K + 5, sub_rate=0.0)
    for j, r in enumerate(base):
        pos = 100 - 1 - int(rng.integers(0, K)) if j % 2 == 0 else int(rng.integers(0, 100 - K))
        reads.append(r[:pos] + b"N" + r[pos + 1:])
    # text prefixes: toeholds at the text's start that wrap below zero, as hits of the table
    for m in (K, K + 1, K + 8, 100):
        reads.append(text[:m])
    reads += [text[-m:] for m in (K, K + 3, 90)]
    reads += [b"", b"A", b"ACGT", b"acgt" * (K // 4 + 1), b"A" * (K + 1)]
    return reads


@pytest.mark.parametrize("K", [16, 20, 44, 52, 60])
def test_jump_table_bit_exact(synth, K):
    """lo / hi / toehold, counts and locations (max_hits 0, 1, 3, 2^64 - 1) with the table equal the oracle's and those without it;
    rbg_layout_info is identical with the table on and off; a replica answers identically."""
    S = synth
    off_rb = _load(S, 0)
    rb = _load(S, K)
    ji = rb.jump_info()
    assert off_rb.jump_info().k == 0 and off_rb.jump_info().keys == 0
    assert ji.k == K and ji.keys > 0 and ji.buckets >= ji.keys and ji.bytes == 64 * ji.buckets and ji.build_ms > 0
    assert bytes(rb.layout_info()) == bytes(off_rb.layout_info())
    assert int(rb.info().hbm_bytes) >= int(off_rb.info().hbm_bytes) + ji.bytes
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    reads = _reads(S, K)
    seqs, off = ra.pack_reads(reads)
    wlo, whi, wk = o.find_range_w_toehold_batch(seqs, off)
    assert (wlo <= whi).sum() > 2000 and (wlo > whi).sum() > 200          # (hits and misses both present)
    lo, hi, k = rb.find_range_w_toehold(seqs, off)
    assert (lo == wlo).all() and (hi == whi).all() and (k == wk).all()
    lo1, hi1 = rb.find_range(seqs, off)
    assert (lo1 == wlo).all() and (hi1 == whi).all()
    want_count = np.where(wlo <= whi, whi - wlo + np.uint64(1), np.uint64(0))
    assert (np.asarray(rb.count(seqs, off), dtype=np.uint64) == want_count).all()
    l0, h0, k0 = off_rb.find_range_w_toehold(seqs, off)
    assert (l0 == lo).all() and (h0 == hi).all() and (k0 == k).all()
    # the instrumented search, toehold and count forms: same answers; with the table far fewer LF steps for the same symbols
    for toe in (True, False):
        dlo, dhi, dk, st_on = _dev_search(rb, seqs, off, toe)
        _, _, _, st_off = _dev_search(off_rb, seqs, off, toe)
        assert (dlo == wlo).all() and (dhi == whi).all() and (not toe or (dk == wk).all())
        hits = int(((wlo <= whi) & (np.diff(off) >= K)).sum())
        assert st_on[ST_STEPS] <= st_off[ST_STEPS] and st_on[ST_FTAB] >= hits   # (K = 16 saves no step of a 100 bp read: 16 + 84 vs 12 + 88)
        assert st_off[ST_STEPS] - st_on[ST_STEPS] >= hits * ((K - 12) // 8) // 2, (K, hits, st_on, st_off)
    for max_hits in (0, 1, 3, MAXU):
        loc_off, locs = rb.locs_at(lo, hi, k, max_hits)
        woff, wlocs = o.locs_at_batch(wlo, whi, wk, max_hits)
        assert (loc_off == woff).all() and (locs == wlocs).all()
    rep = rb.replicate(0)
    try:
        assert rep.jump_info().k == K and rep.jump_info().buckets == ji.buckets
        l2, h2, k2 = rep.find_range_w_toehold(seqs, off)
        assert (l2 == wlo).all() and (h2 == whi).all() and (k2 == wk).all()
    finally:
        rep.close()
    rb.close()
    off_rb.close()
    o.close()


@pytest.mark.parametrize("K", [16, 52, 60])
def test_jump_table_answers_reads_of_exactly_k_symbols_by_the_probe_alone(synth, K):
    """reads of exactly K symbols that occur: with the table every one is answered by its probe -- no LF step at all, K symbols consumed per
    read -- and bit-exact (toehold and count forms, locations); without it they take the ftab and the steps"""
    S = synth
    rb, off_rb = _load(S, K), _load(S, 0)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    text = S.text.tobytes()
    reads = S.sample_reads(1500, K, seed=100 + K, sub_rate=0.0) + [text[:K]]     # (text[:K]: its toehold is text position 0 - wraps below zero after it)
    seqs, off = ra.pack_reads(reads)
    N = len(reads)
    wlo, whi, wk = o.find_range_w_toehold_batch(seqs, off)
    assert (wlo <= whi).all()
    for toe in (True, False):
        lo, hi, k, st = _dev_search(rb, seqs, off, toe)
        assert (lo == wlo).all() and (hi == whi).all() and (not toe or (k == wk).all())
        assert st[ST_STEPS] == 0 and st[ST_SYMBOLS] == N * K and N <= st[ST_FTAB] <= 3 * N, st
        _, _, _, st0 = _dev_search(off_rb, seqs, off, toe)
        assert st0[ST_STEPS] >= N * ((K - 12) // 8), st0
    lo, hi, k = rb.find_range_w_toehold(seqs, off)
    assert (lo == wlo).all() and (hi == whi).all() and (k == wk).all()
    for max_hits in (0, 1, 3, MAXU):
        loc_off, locs = rb.locs_at(lo, hi, k, max_hits)
        woff, wlocs = o.locs_at_batch(wlo, whi, wk, max_hits)
        assert (loc_off == woff).all() and (locs == wlocs).all()
    rb.close()
    off_rb.close()
    o.close()


def test_jump_table_golden_index(data_dir):
    """the reference's toy fixture (a golden index): the table on it answers like the oracle and the reference's golden range"""
    prefix = os.path.join(data_dir, "small.fa")
    ra.set_default_option(capi.OPT_RANK_LAYOUT, capi.LAYOUT_RUNS)
    try:
        with capi.default_option(capi.OPT_JUMP_K, 16):
            rb = ra.load_rowbowt(prefix, ra.LoadRbwtFlag.SA, device=0)
    finally:
        ra.set_default_option(capi.OPT_RANK_LAYOUT, capi.LAYOUT_AUTO)
    o = orc.Oracle.load(prefix, orc.SA)
    reads = orc.read_fastx(os.path.join(data_dir, "simple_query.fq"))[1] + orc.read_fastx(os.path.join(data_dir, "error_query.fq"))[1]
    seqs, off = ra.pack_reads(reads)
    wlo, whi, wk = o.find_range_w_toehold_batch(seqs, off)
    lo, hi, k = rb.find_range_w_toehold(seqs, off)
    assert (lo == wlo).all() and (hi == whi).all() and (k == wk).all()
    assert (int(lo[0]), int(hi[0])) == (24279, 24280)                    # reference tests/rb_tests.cpp:115
    loc_off, locs = rb.locs_at(lo, hi, k)
    woff, wlocs = o.locs_at_batch(wlo, whi, wk)
    assert (loc_off == woff).all() and (locs == wlocs).all()
    assert rb.jump_info().k == 16 and rb.jump_info().keys > 0
    _, _, _, st = _dev_search(rb, seqs, off, True)
    assert st[ST_SYMBOLS] > 0 and st[ST_FTAB] > 0
    rb.close()
    o.close()


def test_jump_table_skipped_at_8_byte_positions_and_by_default_on_small_indexes(synth):
    """8-byte positions: no table (rbg_jump_info all zero); the automatic setting builds none for a replica that fits the cache"""
    S = synth
    rb8 = _load(S, 52, pos_bytes=8)
    assert rb8.info().pos_bytes == 8 and rb8.jump_info().k == 0 and rb8.jump_info().bytes == 0
    rb8.close()
    assert capi.get_default_option(capi.OPT_JUMP_K) == -1
    rb = _with_layout(capi.LAYOUT_RUNS, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    assert rb.jump_info().k == 0
    rb.close()
