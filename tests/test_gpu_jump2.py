"""GPU parity of level 2 of the jump table (RBG_OPT_JUMP2_K; rbg_jump.h, k_jump.hip, k_runs.hip): after a hit of the first table a staged read
with K2 more symbols looks {those symbols, its lo} up in a second table, so that a read of K1 + K2 symbols takes no step at all.  Bit-exact
lo / hi / toehold against the oracle with both tables, with level 2 off and with both off; the instrumented search (rbg_find_range_stats_dev)
shows which path answered: its sums count the buckets of either level in ST_FTAB and the symbols either level consumed in ST_SYMBOLS, and the
steps that remain are exactly those of the symbols the tables did not consume.  The probe lives in the staged byte-form walk, so every query
goes there (OPT_PACKED_READS = 0)."""
import contextlib

import numpy as np
import pytest

import orc
import rowbowt_amd as ra
from rowbowt_amd import capi
from gpu_common import _with_layout

pytestmark = pytest.mark.gpu
ST_STEPS, ST_FTAB, ST_SYMBOLS = 0, 4, 7      # rbg_dev.h kStSteps, kStFtab (ftab entries + probed buckets), kStSymbols
K1 = 16      # the issue's K1; one more case crosses the 64-symbol chunk of a word and a key that starts inside a staged word


@pytest.fixture(autouse=True)
def _byte_form():
    with capi.default_option(capi.OPT_PACKED_READS, 0):
        yield


def _load(S, k1, k2, more=None):
    opts = {capi.OPT_JUMP_K: k1, capi.OPT_JUMP2_K: k2}
    opts.update(more or {})
    with contextlib.ExitStack() as st:
        for o, v in opts.items():
            st.enter_context(capi.default_option(o, v))
        return _with_layout(capi.LAYOUT_RUNS, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))


def _dev_search(rb, reads, toehold=True):
    """rbg_find_range_stats_dev on device arrays: (lo, hi, k or None, the instrumented sums)"""
    import torch
    seqs, off = ra.pack_reads(reads)
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


def _clean_reads(S, K2, n_each=150, K1=K1):
    """reads sampled from the text, no substitution: the five lengths around K1 + K2, and text prefixes (toeholds that wrap below zero)"""
    T = K1 + K2
    text = S.text.tobytes()
    reads = []
    for m in (T - 1, T, T + 1, T + 8, T + 9):
        reads += S.sample_reads(n_each, m, seed=1000 + K2 + m, sub_rate=0.0)
        reads.append(text[:m])
    return reads


def _broken_reads(S, K2, K1=K1):
    T = K1 + K2
    rng = np.random.default_rng(77 + K2)
    other = lambda c: bytes([[x for x in b"ACGT" if x != c][int(rng.integers(3))]])
    reads = []
    for j, r in enumerate(S.sample_reads(300, T + 9, seed=2000 + K2, sub_rate=0.0)):
        m = len(r)
        if j % 3 == 0:      # a substitution inside the K2 symbols of level 2: level 1 hits, level 2 is absent, the steps go on
            pos = m - 1 - K1 - int(rng.integers(0, K2))
            reads.append(r[:pos] + other(r[pos]) + r[pos + 1:])
        elif j % 3 == 1:    # ... inside the last K1: level 1 misses
            pos = m - 1 - int(rng.integers(0, K1))
            reads.append(r[:pos] + other(r[pos]) + r[pos + 1:])
        else:               # a symbol outside the alphabet: the wave walks bytes
            pos = int(rng.integers(0, m))
            reads.append(r[:pos] + b"N" + r[pos + 1:])
    reads += [b"", b"A", b"ACGT" * (T // 4 + 2), b"A" * (T + 1)]
    return reads


@pytest.fixture(scope="module")
def oracle(synth):
    o = orc.Oracle.from_runs(synth.heads, synth.lens, synth.ssa, synth.esa)
    yield o
    o.close()


@pytest.fixture(scope="module")
def plain(synth):
    """neither table, no ftab: every symbol of a read is consumed by a step"""
    with capi.default_option(capi.OPT_PACKED_READS, 0):
        rb = _load(synth, 0, 0, {capi.OPT_FTAB_K: 0})
    yield rb
    rb.close()


# (16, .): the issue's cases, words of at most 64 symbols.  (36, 48): 84 symbols -- the word's second packed chunk in the build (k_jump_keep,
# the packed search of two chunks, k_jump_insert's key from words 2..5) and a level-2 key that starts 8 symbols into a staged word (the funnel
# shift of jump_key_from_codes in the kernel).  (60, 40): the shipped default.
@pytest.mark.parametrize("K1,K2", [(16, 16), (16, 40), (16, 48), (36, 48), (60, 40)])
def test_jump2_bit_exact_and_answers_by_its_probe(synth, oracle, plain, K1, K2):
    S, o, T = synth, oracle, K1 + K2
    both, l1, off = _load(S, K1, K2), _load(S, K1, 0), _load(S, 0, 0)
    try:
        ji, j1 = both.jump_info(), l1.jump_info()
        assert (ji.k, ji.k2) == (K1, K2) and ji.keys2 > 0 and ji.buckets2 >= ji.keys2 and ji.bytes2 == 64 * ji.buckets2 and ji.build2_ms > 0
        assert (j1.k, j1.k2, j1.keys2, j1.bytes2) == (K1, 0, 0, 0) and (ji.keys, ji.bytes) == (j1.keys, j1.bytes)
        assert off.jump_info().k == 0 and off.jump_info().k2 == 0
        assert bytes(both.layout_info()) == bytes(off.layout_info()) == bytes(l1.layout_info())
        assert int(both.info().hbm_bytes) >= int(l1.info().hbm_bytes) + ji.bytes2
        old = capi.JumpInfo()                                       # the call of before level 2 writes its five fields and no more
        old.k2 = 12345
        import ctypes
        assert ra.lib().rbg_jump_info(both.h, ctypes.byref(old)) == 0 and old.k == K1 and old.k2 == 12345
        clean, broken = _clean_reads(S, K2, K1=K1), _broken_reads(S, K2, K1=K1)
        mixed = clean + broken
        order = np.random.default_rng(K2).permutation(len(mixed))   # every kind within one wave
        mixed = [mixed[i] for i in order]
        # (a wave with one symbol outside the alphabet walks bytes and probes nothing: the batch without those reads is the one whose waves are staged)
        for batch in ([r for r in mixed if b"N" not in r], mixed):
            seqs, offs = ra.pack_reads(batch)
            wlo, whi, wk = o.find_range_w_toehold_batch(seqs, offs)
            assert (wlo <= whi).sum() >= len(clean) and (wlo > whi).sum() >= 100
            for rb in (both, l1, off):
                lo, hi, k = rb.find_range_w_toehold(seqs, offs)
                assert (lo == wlo).all() and (hi == whi).all() and (k == wk).all()
                lo1, hi1 = rb.find_range(seqs, offs)
                assert (lo1 == wlo).all() and (hi1 == whi).all()
                for toe in (True, False):
                    dlo, dhi, dk, _ = _dev_search(rb, batch, toe)
                    assert (dlo == wlo).all() and (dhi == whi).all() and (not toe or (dk == wk).all())
        loc_off, locs = both.locs_at(wlo, whi, wk)
        woff, wlocs = o.locs_at_batch(wlo, whi, wk)
        assert (loc_off == woff).all() and (locs == wlocs).all()
        # which path answered.  Clean reads of at least K1 + K2 symbols: every one is answered by level 2 -- the steps left are exactly the
        # steps of the symbols before the last K1 + K2 (measured on the index without tables or ftab), all symbols are consumed, and each
        # read fetched at least one bucket of each level.  With level 2 off the same holds for K1.
        full = [r for r in clean if len(r) >= T]
        cs, co = ra.pack_reads(full)
        flo, fhi, fk = o.find_range_w_toehold_batch(cs, co)
        assert (flo <= fhi).all()
        nsym = sum(len(r) for r in full)
        for toe in (True, False):
            lo, hi, k, st2 = _dev_search(both, full, toe)
            assert (lo == flo).all() and (hi == fhi).all() and (not toe or (k == fk).all())
            _, _, _, rest2 = _dev_search(plain, [r[:len(r) - T] for r in full], toe)
            assert st2[ST_STEPS] == rest2[ST_STEPS] and st2[ST_SYMBOLS] == nsym and 2 * len(full) <= st2[ST_FTAB] <= 6 * len(full), (st2, rest2)
            _, _, _, st1 = _dev_search(l1, full, toe)
            _, _, _, rest1 = _dev_search(plain, [r[:len(r) - K1] for r in full], toe)
            assert st1[ST_STEPS] == rest1[ST_STEPS] and st1[ST_SYMBOLS] == nsym and len(full) <= st1[ST_FTAB] <= 3 * len(full), (st1, rest1)
            assert st2[ST_STEPS] < st1[ST_STEPS]
        # reads of exactly K1 + K2 symbols execute zero steps
        exact = [r for r in clean if len(r) == T]
        assert len(exact) > 100
        for toe in (True, False):
            _, _, _, st = _dev_search(both, exact, toe)
            assert st[ST_STEPS] == 0 and st[ST_SYMBOLS] == T * len(exact), st
        # one symbol short of K1 + K2: level 1 answers, level 2 is not probed
        short = [r for r in clean if len(r) == T - 1]
        _, _, _, st = _dev_search(both, short)
        _, _, _, st_l1 = _dev_search(l1, short)
        # (the buckets a probe reads depend on the order the build's atomics filled the table in: bounded, not compared between two builds)
        assert st[ST_STEPS] == st_l1[ST_STEPS] > 0 and st[ST_SYMBOLS] == st_l1[ST_SYMBOLS] == (T - 1) * len(short)
        assert len(short) <= st[ST_FTAB] <= 3 * len(short) and len(short) <= st_l1[ST_FTAB] <= 3 * len(short)
        # a replica answers identically, from its own copies of both tables
        rep = both.replicate(0)
        try:
            rj = rep.jump_info()
            assert (rj.k, rj.k2, rj.buckets, rj.buckets2, rj.keys2) == (K1, K2, ji.buckets, ji.buckets2, ji.keys2)
            l2, h2, k2 = rep.find_range_w_toehold(seqs, offs)
            assert (l2 == wlo).all() and (h2 == whi).all() and (k2 == wk).all()
            _, _, _, st = _dev_search(rep, exact)
            assert st[ST_STEPS] == 0
        finally:
            rep.close()
    finally:
        both.close()
        l1.close()
        off.close()


def test_jump2_exists_only_where_level_1_does_and_is_off_unless_asked(synth):
    """no level 1, no level 2; level 1 asked for by its K leaves the automatic level 2 off (it belongs to the automatic level 1 at its default K)"""
    S = synth
    rb = _load(S, 0, 40)
    assert rb.jump_info().k == 0 and rb.jump_info().k2 == 0 and rb.jump_info().bytes2 == 0
    rb.close()
    rb = _load(S, K1, -1)
    assert rb.jump_info().k == K1 and rb.jump_info().k2 == 0
    rb.close()
    rb = _load(S, -1, -1)                       # (a replica that fits the cache: neither)
    assert rb.jump_info().k == 0 and rb.jump_info().k2 == 0
    rb.close()


def test_jump2_budget_too_small_leaves_level_1_and_the_layout(synth, oracle):
    """HBM budgets from too small for either table to enough for both, 1 MB apart: the layout is the one the same budget gives without tables,
    level 2 appears only on top of level 1, some budget holds level 1 and not level 2, some holds both, and whatever was built answers like the oracle"""
    S, o = synth, oracle
    reads = _clean_reads(S, 48, n_each=40) + _broken_reads(S, 48)[:60]
    seqs, offs = ra.pack_reads(reads)
    wlo, whi, wk = o.find_range_w_toehold_batch(seqs, offs)
    seen = []
    for mb in range(1, 17):
        base = _load(S, 0, 0, {capi.OPT_HBM_BUDGET_MB: mb})
        rb = _load(S, K1, 48, {capi.OPT_HBM_BUDGET_MB: mb})
        try:
            ji = rb.jump_info()
            assert bytes(rb.layout_info()) == bytes(base.layout_info())
            assert ji.k in (0, K1) and ji.k2 in (0, 48) and (ji.k2 == 0 or ji.k == K1)
            assert int(rb.info().hbm_bytes) == int(base.info().hbm_bytes) + ji.bytes + ji.bytes2
            lo, hi, k = rb.find_range_w_toehold(seqs, offs)
            assert (lo == wlo).all() and (hi == whi).all() and (k == wk).all()
            seen.append((int(ji.k), int(ji.k2)))
        finally:
            rb.close()
            base.close()
    assert (K1, 0) in seen and (K1, 48) in seen, seen
    # (not monotone in the budget: a larger budget also keeps more of the layout, which can leave the tables less room)
