"""GPU parity of the early end at the jump probe (rbg_jump.h jump_complete_mask; k_runs.hip): where a level of the jump table is complete --
every word that occurs is in it -- a staged read whose key the level lacks ends at the probe with the empty range instead of walking the ftab path
to the same answer.  Bit-exact lo / hi / toehold against the oracle, against the same library with the switch off (RBG_JUMP_ABSENT_ENDS=0) and
against the library without tables, through rbg_find_range_w_toehold_dev and rbg_find_range_dev, with equal counters; what rbg_jump_info_sized
reports as complete; the instrumented search unchanged by the switch and still walking; a replica of rbg_replicate_many; a load from a cache file.
The probe lives in the STAGED byte-form walk: every query goes to the byte form (OPT_PACKED_READS = 0), and all but three named waves of the batch
hold nothing but ACGT reads the staging takes (_staged_waves), which the instrumented sums confirm on the device (probed buckets, fewer steps)."""
import contextlib
import os

import numpy as np
import pytest

import orc
import rowbowt_amd as ra
from rowbowt_amd import capi
from gpu_common import _with_layout

pytestmark = pytest.mark.gpu
ST_STEPS, ST_FTAB, ST_SYMBOLS = 0, 4, 7      # rbg_dev.h kStSteps, kStFtab (ftab entries + probed buckets), kStSymbols
STAGE_CAP = 256      # rbg_runs_device.hpp kStageCap: a wave holding a longer read walks bytes


@pytest.fixture(autouse=True)
def _byte_form():
    with capi.default_option(capi.OPT_PACKED_READS, 0):
        yield


def _load(S, k1, k2, absent_ends=True, more=None):
    """run-indexed, 4-byte positions, the tables asked for by their K; absent_ends=False: the load sees RBG_JUMP_ABSENT_ENDS=0"""
    opts = {capi.OPT_JUMP_K: k1, capi.OPT_JUMP2_K: k2}
    opts.update(more or {})
    before = os.environ.pop("RBG_JUMP_ABSENT_ENDS", None)
    if not absent_ends:
        os.environ["RBG_JUMP_ABSENT_ENDS"] = "0"
    try:
        with contextlib.ExitStack() as st:
            for o, v in opts.items():
                st.enter_context(capi.default_option(o, v))
            return _with_layout(capi.LAYOUT_RUNS, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    finally:
        os.environ.pop("RBG_JUMP_ABSENT_ENDS", None)
        if before is not None:
            os.environ["RBG_JUMP_ABSENT_ENDS"] = before


class _Batch:
    """one batch on the device, searched through the *_dev entry points"""

    def __init__(self, reads):
        import torch
        self.torch = torch
        seqs, off = ra.pack_reads(reads)
        self.seqs, self.off, self.N = seqs, off, len(off) - 1
        dev = torch.device("cuda:0")
        self.d_seqs = torch.from_numpy(np.concatenate([seqs, np.zeros((-len(seqs)) % 16 + 16, np.uint8)])).to(dev)
        self.d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        self.out = [torch.empty(self.N, dtype=torch.int64, device=dev) for _ in range(3)]
        self.d_st = torch.zeros(16, dtype=torch.int64, device=dev)

    def _u(self, t):
        return t.cpu().numpy().view(np.uint64).copy()

    def search(self, rb, toehold):
        """(lo, hi, k or None, the counters this one launch added)"""
        torch, L = self.torch, ra.lib()
        for t in self.out:
            t.fill_(-7)
        st = torch.cuda.current_stream().cuda_stream
        rb.counters_reset()
        d_lo, d_hi, d_k = self.out
        if toehold:
            rc = L.rbg_find_range_w_toehold_dev(rb.h, self.d_seqs.data_ptr(), self.d_off.data_ptr(), self.N, d_lo.data_ptr(), d_hi.data_ptr(), d_k.data_ptr(), st)
        else:
            rc = L.rbg_find_range_dev(rb.h, self.d_seqs.data_ptr(), self.d_off.data_ptr(), self.N, d_lo.data_ptr(), d_hi.data_ptr(), st)
        assert rc == 0
        torch.cuda.synchronize()
        return self._u(d_lo), self._u(d_hi), (self._u(d_k) if toehold else None), rb.counters()[:3].tolist()

    def stats(self, rb, toehold):
        torch = self.torch
        self.d_st.zero_()
        d_lo, d_hi, d_k = self.out
        rc = ra.lib().rbg_find_range_stats_dev(rb.h, self.d_seqs.data_ptr(), self.d_off.data_ptr(), self.N, d_lo.data_ptr(), d_hi.data_ptr(),
                                              d_k.data_ptr() if toehold else None, self.d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        return self._u(d_lo), self._u(d_hi), self.d_st.cpu().numpy().tolist()


LOWER_WAVE, N_WAVE, CAP_WAVE = 11, 3, 7      # the waves (64-read slices of the batch) that walk bytes: every other one is staged


def _reads(S, K1, K2):
    """about 900 reads, not a multiple of 64, every kind of the early end's neighbourhood shuffled through every wave.  Three waves walk bytes and probe
    nothing: N_WAVE holds a read with N, CAP_WAVE one longer than the staging holds, LOWER_WAVE the lowercase reads (no symbols of this alphabet); all
    the other waves hold ACGT reads of at most STAGE_CAP symbols and are staged.  Returns (reads, kind of each read)."""
    T = K1 + K2
    rng = np.random.default_rng(1000 * K1 + K2)
    text = S.text.tobytes()
    other = lambda c: bytes([[x for x in b"ACGT" if x != c][int(rng.integers(3))]])
    sub = lambda r, pos: r[:pos] + other(r[pos]) + r[pos + 1:]
    reads, kinds = [], []

    def add(kind, rs):
        reads.extend(rs)
        kinds.extend([kind] * len(rs))

    for j, m in enumerate((K1, T - 1, T, T + 20)):                  # clean: the last walks on after level 2 hit
        add("clean%d" % j, S.sample_reads(100, m, seed=10 * T + j, sub_rate=0.0))
    long_ = S.sample_reads(390, T + 20, seed=10 * T + 5, sub_rate=0.0)
    add("absent1", [sub(r, len(r) - 1 - int(rng.integers(0, K1))) for r in long_[:130]])            # in the last K1 symbols: absent at level 1
    add("absent2", [sub(r, len(r) - 1 - K1 - int(rng.integers(0, K2))) for r in long_[130:260]])    # in the K2 before them: level 1 hits, absent at level 2
    add("walk_empties", [sub(r, int(rng.integers(0, 20))) for r in long_[260:]])                    # in the first 20: both levels hit, the walk empties
    add("short", S.sample_reads(90, K1 - 1, seed=10 * T + 6, sub_rate=0.2) + [b"", b"A", b"ACGT"])
    # the match ends at text position 0 (the first 120 symbols occur nowhere else: the toehold is position 0 itself, the next step would wrap below it)
    add("text_start", [text[:m] for m in (K1, T - 1, T, T + 20, 120)])
    order = rng.permutation(len(reads))
    reads, kinds = [reads[i] for i in order], [kinds[i] for i in order]
    with_n = S.sample_reads(1, T + 20, seed=10 * T + 8, sub_rate=0.0)[0]
    special = [(64 * N_WAVE + 5, "with_n", with_n[:7] + b"N" + with_n[8:]), (64 * CAP_WAVE + 9, "over_cap", text[100:100 + STAGE_CAP + 44])]
    special += [(64 * LOWER_WAVE + 3 * j, "lowercase", r.lower()) for j, r in enumerate(S.sample_reads(20, T + 20, seed=10 * T + 7, sub_rate=0.0))]
    for at, kind, r in sorted(special):                              # (ascending: an insert moves only what lies behind it)
        reads.insert(at, r)
        kinds.insert(at, kind)
    assert len(reads) % 64 != 0 and 900 <= len(reads) <= 1100
    return reads, np.array(kinds)


def _staged_waves(reads, kinds):
    """the waves of the batch the kernel stages (every read of the 64-read slice over ACGT, none above STAGE_CAP), checked to be all but the three
    named ones and to mix, each of them, clean reads with the three kinds of reads that end empty"""
    nw = (len(reads) + 63) // 64
    staged = [all(len(r) <= STAGE_CAP and not r.translate(None, b"ACGT") for r in reads[64 * w:64 * w + 64]) for w in range(nw)]
    assert [w for w in range(nw) if not staged[w]] == sorted((N_WAVE, CAP_WAVE, LOWER_WAVE)) and nw >= 15
    for w in range(nw):
        in_w = set(kinds[64 * w:64 * w + 64].tolist())
        if staged[w] and 64 * w + 64 <= len(reads):                 # (the last, partial wave holds what the shuffle left it)
            assert {"absent1", "absent2", "walk_empties", "clean0", "clean3"} <= in_w and ({"clean1", "clean2"} & in_w), (w, in_w)
    return [w for w in range(nw) if staged[w]]


def _probes_and_ftab_entries(o, reads, K1, K2, ftab_k):
    """what the instrumented search of STAGED reads must count, from the oracle alone: P = probes (level 1: the read has K1 symbols; level 2: its last K1
    occur and K2 more are left), F = ftab entries fetched (no hit of level 1 and ftab_k symbols: the ftab path).  K1 = 0: no table, every read of ftab_k."""
    tails = [r[len(r) - K1:] if K1 and len(r) >= K1 else b"" for r in reads]
    seqs, off = ra.pack_reads(tails)
    tlo, thi, _ = o.find_range_w_toehold_batch(seqs, off)
    P = F = 0
    for i, r in enumerate(reads):
        hit1 = bool(K1) and len(r) >= K1 and tlo[i] <= thi[i]
        P += (1 if K1 and len(r) >= K1 else 0) + (1 if hit1 and K2 and len(r) - K1 >= K2 else 0)
        F += 1 if not hit1 and ftab_k and len(r) >= ftab_k else 0
    return P, F


@pytest.fixture(scope="module")
def oracle(synth):
    o = orc.Oracle.from_runs(synth.heads, synth.lens, synth.ssa, synth.esa)
    yield o
    o.close()


# (16, 16): the smallest keys allowed.  (36, 48): a level-2 key that starts inside a staged word.
@pytest.mark.parametrize("K1,K2", [(16, 16), (36, 48)])
def test_absent_keys_end_reads_bit_exactly(synth, oracle, K1, K2):
    S, o = synth, oracle
    reads, kinds = _reads(S, K1, K2)
    staged = _staged_waves(reads, kinds)
    B = _Batch(reads)
    wlo, whi, wk = o.find_range_w_toehold_batch(B.seqs, B.off)
    empty = wlo > whi
    # the batch holds what it is meant to: reads the levels end, reads that hit and go on, reads the walk empties
    assert empty[kinds == "absent1"].sum() >= 100 and empty[kinds == "absent2"].sum() >= 100 and empty[kinds == "walk_empties"].sum() >= 100
    for j in range(4):
        assert not empty[kinds == "clean%d" % j].any()
    assert not empty[kinds == "text_start"].any() and (wk[kinds == "text_start"] == 0).any()
    assert empty[kinds == "lowercase"].all() and empty[kinds == "with_n"].all() and not empty[kinds == "over_cap"].any()
    on, sw_off, none = _load(S, K1, K2), _load(S, K1, K2, absent_ends=False), _load(S, 0, 0)
    try:
        ji = on.jump_info()
        assert (ji.k, ji.k2) == (K1, K2) and on.jump_complete() == 3
        jo = sw_off.jump_info()
        assert (jo.k, jo.k2, jo.keys, jo.keys2) == (K1, K2, ji.keys, ji.keys2) and sw_off.jump_complete() == 0
        assert none.jump_info().k == 0 and none.jump_complete() == 0
        want_counters = [B.N, int((~empty).sum()), int((whi[~empty] - wlo[~empty] + np.uint64(1)).sum())]
        for rb in (on, sw_off, none):
            lo, hi, k, c = B.search(rb, True)
            assert (lo == wlo).all() and (hi == whi).all() and (k == wk).all()
            assert c == want_counters
            lo, hi, _, c = B.search(rb, False)
            assert (lo == wlo).all() and (hi == whi).all()
            assert c == want_counters
            lo, hi, k = rb.find_range_w_toehold(B.seqs, B.off)     # (the host path: the same kernel behind its own staging of the batch)
            assert (lo == wlo).all() and (hi == whi).all() and (k == wk).all()
        # The instrumented search keeps walking (trap one).  On the whole batch: the same answers and the same sums with the switch on and off, but for
        # slot 4 (ftab entries + probed buckets): a key's chain depends on the order the build's atomics filled the table in, and these are two builds.
        for toe in (True, False):
            lo1, hi1, st_on = B.stats(on, toe)
            lo0, hi0, st_off = B.stats(sw_off, toe)
            assert (lo1 == wlo).all() and (hi1 == whi).all() and (lo0 == wlo).all() and (hi0 == whi).all()
            assert [v for t, v in enumerate(st_on) if t != ST_FTAB] == [v for t, v in enumerate(st_off) if t != ST_FTAB], (st_on, st_off)
        # On the staged waves alone slot 4 is pinned from the oracle: F ftab entries (the reads without a hit of level 1 -- the absent ones among them,
        # which an instrumented kernel that ended them would not count) and between one and three buckets for each of the P probes (a table at most
        # half full: the bound of tests/test_gpu_jump2.py), with either switch; without tables every read takes its ftab entry and more steps.
        ftab_k = int(on.info().ftab_k)
        assert 0 < ftab_k < K1
        staged_reads = [r for w in staged for r in reads[64 * w:64 * w + 64]]
        SB = _Batch(staged_reads)
        P, F = _probes_and_ftab_entries(o, staged_reads, K1, K2, ftab_k)
        _, F0 = _probes_and_ftab_entries(o, staged_reads, 0, 0, ftab_k)
        assert P > 1.2 * len(staged_reads) and F > 150
        for toe in (True, False):
            _, _, s_on = SB.stats(on, toe)
            _, _, s_off = SB.stats(sw_off, toe)
            _, _, s_none = SB.stats(none, toe)
            print(f"staged waves K1={K1} K2={K2} toehold={toe}: F={F} P={P} F0={F0} on={s_on[:8]} off={s_off[:8]} none={s_none[:8]}")
            assert [v for t, v in enumerate(s_on) if t != ST_FTAB] == [v for t, v in enumerate(s_off) if t != ST_FTAB], (s_on, s_off)
            assert F + P <= s_on[ST_FTAB] <= F + 3 * P and F + P <= s_off[ST_FTAB] <= F + 3 * P, (F, P, s_on, s_off)
            assert s_none[ST_FTAB] == F0 and s_none[ST_STEPS] > s_on[ST_STEPS] > 0, (s_none, s_on)
        # Reads that miss level 1 walk exactly as they do without a table -- ftab entry, then steps until the range empties: two full staged waves of
        # them give the same sums with the switch on, off and without tables (slot 4: one ftab entry each, plus the probe's one to three buckets)
        tails = ra.pack_reads([r[len(r) - K1:] for r in reads])      # (a substituted K1-mer can still occur elsewhere: the oracle says which do not)
        tlo, thi, _ = o.find_range_w_toehold_batch(*tails)
        missing = [r for r, kd, t in zip(reads, kinds, tlo > thi) if kd == "absent1" and t][:128]
        assert len(missing) == 128
        AB = _Batch(missing)
        Pm, Fm = _probes_and_ftab_entries(o, missing, K1, K2, ftab_k)
        assert (Pm, Fm) == (128, 128)
        for toe in (True, False):
            _, _, a_on = AB.stats(on, toe)
            _, _, a_off = AB.stats(sw_off, toe)
            _, _, a_none = AB.stats(none, toe)
            print(f"level-1 misses K1={K1} K2={K2} toehold={toe}: on={a_on[:8]} off={a_off[:8]} none={a_none[:8]}")
            rest = lambda st: [v for t, v in enumerate(st) if t != ST_FTAB]
            assert rest(a_on) == rest(a_off) == rest(a_none) and a_on[ST_STEPS] > 0 and a_on[ST_SYMBOLS] > 0, (a_on, a_off, a_none)
            assert a_none[ST_FTAB] == 128 and 256 <= a_on[ST_FTAB] <= 512 and 256 <= a_off[ST_FTAB] <= 512, (a_on, a_off, a_none)
        # a replica made by rbg_replicate_many on the same device
        rep = on.replicate_many([0])[0]
        try:
            assert rep.jump_complete() == 3
            lo, hi, k, c = B.search(rep, True)
            assert (lo == wlo).all() and (hi == whi).all() and (k == wk).all() and c == want_counters
            lo, hi, _, c = B.search(rep, False)
            assert (lo == wlo).all() and (hi == whi).all() and c == want_counters
        finally:
            rep.close()
    finally:
        on.close()
        sw_off.close()
        none.close()


def test_only_the_levels_that_stand_are_complete(synth, oracle, tmp_path):
    """level 2 switched off: level 1 alone is complete; level 2 declined by the budget: the same; the switch off: neither -- and each answers like the oracle"""
    S, o = synth, oracle
    reads, kinds = _reads(S, 16, 48)
    _staged_waves(reads, kinds)
    B = _Batch(reads)
    wlo, whi, wk = o.find_range_w_toehold_batch(B.seqs, B.off)

    def check(rb, want):
        assert rb.jump_complete() == want, (rb.jump_complete(), want)
        lo, hi, k, _ = B.search(rb, True)
        assert (lo == wlo).all() and (hi == whi).all() and (k == wk).all()

    rb = _load(S, 16, 0)
    assert (rb.jump_info().k, rb.jump_info().k2) == (16, 0)
    check(rb, 1)
    rb.close()
    rb = _load(S, 16, 0, absent_ends=False)
    check(rb, 0)
    rb.close()
    # the cache-load path ends up with the mask as well (RowBowt.from_cache: the same upload, the tables built after it)
    capi.convert_runs(S.heads, S.lens, S.ssa, S.esa, out_path=str(tmp_path / "synth.rbgpu"))
    cached = lambda: ra.RowBowt.from_cache(str(tmp_path / "synth.rbgpu"), ra.LoadRbwtFlag.SA, device=0)
    with capi.default_option(capi.OPT_JUMP_K, 16), capi.default_option(capi.OPT_JUMP2_K, 48):
        rb = _with_layout(capi.LAYOUT_RUNS, cached)
    assert (rb.jump_info().k, rb.jump_info().k2) == (16, 48)
    check(rb, 3)
    rb.close()
    # budgets 1 MB apart (as tests/test_gpu_jump2.py walks them): some hold level 1 and decline level 2
    seen = set()
    for mb in range(1, 17):
        rb = _load(S, 16, 48, more={capi.OPT_HBM_BUDGET_MB: mb})
        try:
            ji = rb.jump_info()
            state = (int(ji.k), int(ji.k2))
            check(rb, {(0, 0): 0, (16, 0): 1, (16, 48): 3}[state])
            seen.add(state)
        finally:
            rb.close()
        if {(16, 0), (16, 48)} <= seen:
            break
    assert (16, 0) in seen, seen
