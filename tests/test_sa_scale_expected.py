"""CPU half of tests/test_gpu_sa_build_scale.py: the inputs of tests/sa_scale_cases.py are where they are meant to be relative to rocPRIM's merge-sort
limit and the grid cap of sa_build.hip, and the counter model (rounds, sorted, tied_after_first from the LCP array) agrees with a second plain
implementation, a numpy simulation of group-head prefix doubling, on small texts.  No device.

The longest common prefix of the near-copies text is asserted from how the text is built, not from a Kasai pass (a Python loop over 3 000 030 positions
takes more than a few seconds, and the suffix array it needs more): copies 1-3 and 5-7 are the sequence itself, so the suffixes at the starts of copies
1 and 5 share 3 * 100 001 - 1 symbols -- a lower bound, which is what "at least 12 rounds" needs.  The vectorised LCP array (lcp_array) that the device
test uses for the exact counters is held here to Kasai's loop on the small texts."""
import numpy as np

import naive
import sa_scale_cases as SC
from sa_scale_cases import CAP, MERGE_LIMIT


def _t(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


def small_cases():
    rng = np.random.default_rng(7)
    T = {"n=1": _t(b"\x01"), "n=2": _t(b"A\x01"), "n=3 zero terminator": _t(b"\x01\x01\x00"), "banana": _t(b"banana\x01")}
    for k in (7, 8, 9, 16, 17, 257, 1030):
        T[f"A*{k}"] = _t(b"A" * k + b"\x01")
    for period, unit in ((4, b"ACGT"), (7, b"ACGTTGA"), (9, b"ACGTTGACA")):
        T[f"period {period}"] = _t((unit * 200)[:1003] + b"\x01")
    for sigma, n in ((2, 1025), (2, 5000), (4, 4097)):
        T[f"sigma {sigma} n {n}"] = np.append(rng.choice(SC.ACGT[:sigma], n - 1), 1).astype(np.uint8)
    base = rng.choice(SC.ACGT, 300)
    copies = [base.copy() for _ in range(9)]
    copies[0][[5, 150]] = ord("N")
    copies[4][[77]] = ord("N")
    T["near copies, small"] = _t(b"#".join(c.tobytes() for c in copies) + b"\x01")
    return T


def kasai(text, sa):
    n = len(text)
    rank = np.empty(n, np.int64)
    rank[sa] = np.arange(n)
    t, s, r = text.tolist(), np.asarray(sa).tolist(), rank.tolist()
    lcp = [0] * (n + 1)
    h = 0
    for i in range(n):
        if r[i] > 0:
            j = s[r[i] - 1]
            while i + h < n and j + h < n and t[i + h] == t[j + h]:
                h += 1
            lcp[r[i]] = h
            if h:
                h -= 1
        else:
            h = 0
    return np.asarray(lcp, np.int64)


def test_every_n_is_where_it_is_meant_to_be():
    assert CAP == 8192 * 256 == 2_097_152 and MERGE_LIMIT == 1_048_576
    assert SC.BOUNDARY_NS == (MERGE_LIMIT, MERGE_LIMIT + 1, CAP - 1, CAP, CAP + 1, 2 * CAP + 1)
    for n in SC.BOUNDARY_NS:
        t = SC.boundary_text(n)
        assert len(t) == n and t[-1] == 1 and (t[:-1] > 1).all() and set(np.unique(t[:-1]).tolist()) == set(b"ACGT")
    passes = lambda n: -(-n // CAP)
    assert [passes(n) for n in SC.BOUNDARY_NS] == [1, 1, 1, 1, 2, 3] and (2 * CAP + 1) - 2 * CAP == 1      # the third pass holds one element
    near = SC.near_copies_at_scale()
    assert len(near) == SC.COPIES * (SC.COPY_LEN + 1) == 3_000_030 and CAP < len(near) < 2 * CAP and near[-1] == 1 and (near[:-1] > 1).all()
    run = SC.long_run()
    assert len(run) == CAP + 301 and passes(len(run)) == 2 and (run[:-1] == ord("A")).all() and run[-1] == 1


def test_near_copies_at_scale_stay_tied_and_take_their_rounds():
    t = SC.near_copies_at_scale()
    unit = SC.COPY_LEN + 1
    # after the first key more suffixes are still listed than one grid pass holds: the later rounds stride the grid too
    assert SC.shared_first_keys(t) > CAP
    # every fourth copy differs from the sequence in about 100 places, the others not at all
    base = t[unit:unit + SC.COPY_LEN]
    for d in range(SC.COPIES):
        differ = int((t[d * unit:d * unit + SC.COPY_LEN] != base).sum())
        assert (90 <= differ <= SC.SNVS) if d % 4 == 0 else differ == 0, (d, differ)
    # the verbatim stretch repeats: copies 1-3 are copies 5-7, '#' included
    stretch = 3 * unit - 1
    assert (t[unit:unit + stretch] == t[5 * unit:5 * unit + stretch]).all()
    assert SC.rounds_of(stretch) >= 12, SC.rounds_of(stretch)


def test_long_run_closed_form():
    for k in (1, 2, 9, 300):
        t = SC.long_run(k)
        sa = SC.long_run_sa(len(t))
        assert (sa == naive.suffix_array(t)).all()
        heads, lens, ssa, esa = SC.runs_from_sa(t, sa)
        assert heads.tolist() == [ord("A"), 1] and lens.tolist() == [k, 1] and ssa.tolist() == [k, 0] and esa.tolist() == [1, 0]
        want = naive.rle(naive.bwt_from_sa(t, sa))
        assert (heads == want[0]).all() and (lens == want[1]).all()
    # at the size the device test uses: all ranks tied up to the last round, every round sorts all but the suffixes that reached the terminator
    t = SC.long_run()
    n = len(t)
    lcp = SC.lcp_array(t, SC.long_run_sa(n))
    assert (lcp[2:n] == np.arange(1, n - 1)).all() and lcp[0] == lcp[1] == lcp[n] == 0
    M = SC.counter_model(t, SC.long_run_sa(n))
    assert M["rounds"] == SC.rounds_of(n - 2) == 20 and M["tied_after_first"] == n - 8, M


def test_runs_from_sa_is_the_naive_run_list():
    for name, t in small_cases().items():
        sa = naive.suffix_array(t)
        bwt = naive.bwt_from_sa(t, sa)
        heads, lens, brk = naive.rle(np.where(bwt == 0, 1, bwt).astype(np.uint8))
        ssa, esa = naive.run_samples(sa, brk, len(t))
        for what, a, b in zip(("heads", "lens", "ssa", "esa"), SC.runs_from_sa(t, sa), (heads, lens, ssa, esa)):
            assert (np.asarray(a).astype(np.uint64) == np.asarray(b).astype(np.uint64)).all(), (name, what)


def test_lcp_array_is_kasais():
    for name, t in small_cases().items():
        sa = naive.suffix_array(t)
        assert (SC.lcp_array(t, sa) == kasai(t, sa)).all(), name


def test_counter_model_against_the_doubling_simulation():
    for name, t in small_cases().items():
        sa = np.asarray(naive.suffix_array(t), np.int64)
        got_sa, counted = SC.doubling_simulation(t)
        assert (got_sa == sa).all(), name
        M = SC.counter_model(t, sa)
        assert M == counted, (name, M, counted)
        assert M["tied_after_first"] == SC.shared_first_keys(t), name
        assert M["rounds"] == SC.rounds_of(int(SC.lcp_array(t, sa).max())), name
    assert SC.counter_model(_t(b"\x01"), np.zeros(1, np.int64)) == dict(rounds=1, sorted=1, tied_after_first=0)
    t = _t(b"A" * 17 + b"\x01")      # lcp 0, 0, 1 .. 16: 10 rows tied at depth 8, 2 at 16, none at 32
    assert SC.counter_model(t, SC.long_run_sa(18)) == dict(rounds=3, sorted=18 + 10 + 2, tied_after_first=10)
