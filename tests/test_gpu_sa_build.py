"""GPU parity of rbg_suffix_array_dev and rbg_text_runs_plan_dev / _fill_dev (rowbowt_amd/csrc/sa_build.hip) against tests/naive.py, exactly, at 4-byte
and at forced 8-byte positions.  d_sa, d_tmp and the run arrays are regions of a guarded arena (tests/arena.py): no byte outside the declared outputs
changes, and the inputs stay as they were.  The texts: the smallest ones, runs of one letter around the first key's width and the wave and workgroup
sizes, periodic strings beside the key width, random texts of 2, 4 and 200 letters (bytes 2 and 255 among them), the 2 051-symbol pangenome, the
documents of extract_wide_cases.docs(), 64 near-copies of one sequence, and one text of two million symbols against the torch suffix array.

The near-copies text is not 64 copies that all differ: with the first key of eight bytes a longest common prefix near 1 000 is sorted out in 8 rounds, not
the ten the case is for.  Every fourth copy carries SNVs and the others are the sequence itself, so stretches of three equal copies repeat, the longest
common prefix passes 3 000 and the rounds are ten; the count is asserted against a Kasai pass over the text (near_copies, rounds_model)."""
import functools
import math

import numpy as np
import pytest
import torch

import naive
import rowbowt_amd as ra
import sa_scale_cases as SC
from rowbowt_amd import capi
from rowbowt_amd.tools import synth_pangenome as SP
from arena import Arena

pytestmark = pytest.mark.gpu
EARG = -4
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _t(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


@functools.lru_cache(maxsize=None)
def near_copies():
    """64 near-copies of a 1 000-base sequence joined by '#': every fourth copy carries three SNVs, the others are the sequence itself, so stretches of
    three equal copies repeat and the longest common prefix passes 3 000 -- with a first key of eight bytes that is at least ten rounds"""
    rng = np.random.default_rng(64)
    base = rng.choice(ACGT, 1000)
    out = []
    for d in range(64):
        s = base.copy()
        if d % 4 == 0:
            for at in rng.choice(1000, 3, replace=False).tolist():
                s[at] = ACGT[(int(np.flatnonzero(ACGT == s[at])[0]) + 1 + int(rng.integers(0, 3))) % 4]
        out.append(s.tobytes())
    return _t(b"#".join(out) + b"\x01")


def max_lcp(text, sa):
    """Kasai"""
    n = len(text)
    rank = np.empty(n, np.int64)
    rank[sa] = np.arange(n)
    t, s, r = text.tolist(), sa.tolist(), rank.tolist()
    h = best = 0
    for i in range(n):
        if r[i] > 0:
            j = s[r[i] - 1]
            while i + h < n and j + h < n and t[i + h] == t[j + h]:
                h += 1
            best = max(best, h)
            if h:
                h -= 1
        else:
            h = 0
    return best


def rounds_model(lcp):
    """the first key sorts by 8 symbols, every further round doubles: the rounds until the depth passes the longest common prefix"""
    rounds, h = 1, 8
    while h <= lcp:
        rounds, h = rounds + 1, h * 2
    return rounds


def small_texts():
    rng = np.random.default_rng(2051)
    T = {"n=1": _t(b"\x01"), "n=2": _t(b"A\x01"), "n=3": _t(b"CA\x01"), "n=3 zero terminator": _t(b"\x01\x01\x00")}
    for k in (1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 4097):
        T[f"A*{k}"] = _t(b"A" * k + b"\x01")
    for period, unit in ((4, b"ACGT"), (7, b"ACGTTGA"), (8, b"ACGTTGAC"), (9, b"ACGTTGACA")):
        for length in range(1000, 1101, 11):
            T[f"period {period} x {length}"] = _t((unit * (length // period + 1))[:length] + b"\x01")
    for sigma in (2, 4, 200):
        letters = ACGT[:sigma] if sigma <= 4 else np.concatenate([[2, 255], rng.choice(np.arange(3, 255), 198, replace=False)]).astype(np.uint8)
        for n in (63, 64, 65, 1023, 1024, 1025, 65535, 65536, 65537):
            t = np.append(rng.choice(letters, n - 1), 1).astype(np.uint8)
            if sigma == 200:
                t[:2] = (2, 255)
            T[f"sigma {sigma} n {n}"] = t
    return T


@functools.lru_cache(maxsize=None)
def texts():
    import extract_wide_cases as EW
    import isa_model as IM
    T = small_texts()
    T["pangenome 2051"] = IM.synth_text().text
    T["docs"] = EW.docs().text
    T["near copies"] = near_copies()
    return T


@functools.lru_cache(maxsize=None)
def expected(name):
    """(sa, heads, lens, ssa, esa) by tests/naive.py: made once per text, shared by both widths"""
    import extract_wide_cases as EW
    import isa_model as IM
    t = texts()[name]
    sa = {"pangenome 2051": lambda: IM.synth_text().sa, "docs": lambda: EW.docs().sa}.get(name, lambda: naive.suffix_array(t))()
    heads, lens, brk = naive.rle(np.where(naive.bwt_from_sa(t, sa) == 0, 1, naive.bwt_from_sa(t, sa)).astype(np.uint8))
    ssa, esa = naive.run_samples(sa, brk, len(t))
    return np.asarray(sa, np.int64), heads, lens, ssa, esa


@functools.lru_cache(maxsize=None)
def counters(name):
    """{rounds, sorted, tied_after_first} of the build by the counter model: once per text, shared by both widths"""
    return SC.counter_model(texts()[name], expected(name)[0])


def run_sa(text, pb, want_rc=0):
    """rbg_suffix_array_dev on a guarded arena -> (rc, the bytes of d_sa, the arena); the text's region and every guard byte are checked"""
    L = ra.lib()
    n = len(text)
    nb = int(L.rbg_sa_tmp_bytes(n, pb))
    A = Arena(n + n * pb + nb + 8192, device="cuda")
    d_text = A.carve_from("text", text, align=1)
    d_sa = A.carve("sa", n * pb, align=pb)
    d_tmp = A.carve("tmp", nb, align=256)
    A.snapshot("text")
    rc = L.rbg_suffix_array_dev(d_text.ptr, n, d_sa.ptr, pb, d_tmp.ptr, nb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    A.check()
    A.assert_all_unchanged()
    return d_sa.numpy(np.uint32 if pb == 4 else np.uint64), A, d_text, d_sa


def run_runs(A, d_text, d_sa, n, pb, R_want):
    L = ra.lib()
    st = torch.cuda.current_stream().cuda_stream
    nb = int(L.rbg_text_runs_tmp_bytes(n, pb))
    B = Arena(nb + 25 * R_want + 8192, device="cuda")
    d_tmp = B.carve("runs tmp", nb, align=256)
    R = capi.U64()
    assert L.rbg_text_runs_plan_dev(d_text.ptr, d_sa.ptr, n, pb, d_tmp.ptr, nb, capi.C.byref(R), st) == 0
    assert int(R.value) == R_want
    heads = B.carve("heads", R_want, align=1)
    lens, ssa, esa = (B.carve(k, R_want * 8, align=8) for k in ("lens", "ssa", "esa"))
    A.snapshot("sa")
    assert L.rbg_text_runs_fill_dev(d_text.ptr, d_sa.ptr, n, pb, d_tmp.ptr, nb, R_want, heads.ptr, lens.ptr, ssa.ptr, esa.ptr, st) == 0
    torch.cuda.synchronize()
    A.check(), B.check(), A.assert_all_unchanged()
    return heads.numpy(), lens.numpy(np.uint64), ssa.numpy(np.uint64), esa.numpy(np.uint64)


def check_info(n, pb):
    info = capi.sa_info()
    assert info["n"] == n and info["pos_bytes"] == pb and info["tmp_bytes"] == ra.lib().rbg_sa_tmp_bytes(n, pb)
    assert 1 <= info["rounds"] <= math.ceil(math.log2(n)) + 1 if n > 1 else info["rounds"] <= 1, info
    assert info["sorted"] <= n * info["rounds"], info
    return info


@pytest.mark.parametrize("pb", [4, 8])
def test_suffix_array_and_runs_of_every_text(pb):
    for name, t in texts().items():
        sa, heads, lens, ssa, esa = expected(name)
        got, A, d_text, d_sa = run_sa(t, pb)
        bad = np.flatnonzero(got.astype(np.int64) != sa)
        assert len(bad) == 0, (name, pb, bad[:5], got[bad[:5]], sa[bad[:5]])
        info = check_info(len(t), pb)
        # exactly what the LCP array says: a suffix leaves the list when no other shares its first 8 * 2^k symbols (sa_scale_cases.counter_model)
        assert {k: info[k] for k in ("rounds", "sorted", "tied_after_first")} == counters(name), (name, pb, info, counters(name))
        if name == "near copies":
            lcp = max_lcp(t, sa)
            assert lcp >= 3000 and rounds_model(lcp) >= 10 and info["rounds"] == rounds_model(lcp), (lcp, info)
            # suffixes that are alone leave the rounds: the terminator's is alone after the first key, so every later round sorts fewer than n
            assert info["tied_after_first"] < len(t) and info["sorted"] <= len(t) + (info["rounds"] - 1) * info["tied_after_first"] < len(t) * info["rounds"], info
        if name.startswith("A*"):
            assert info["rounds"] == rounds_model(len(t) - 2), (name, info)   # all ranks tied up to the last round
        g = run_runs(A, d_text, d_sa, len(t), pb, len(heads))
        for what, a, b in zip(("heads", "lens", "ssa", "esa"), g, (heads, lens, ssa, esa)):
            assert (a == b).all(), (name, pb, what)


def _search_all_runs_text():
    """a text whose BWT has no two equal neighbours (r = n), by search over short random texts"""
    rng = np.random.default_rng(5)
    for _ in range(20000):
        t = np.append(rng.choice(ACGT, 7), 1).astype(np.uint8)
        b = naive.bwt_from_sa(t, naive.suffix_array(t))
        if (b[1:] != b[:-1]).all():
            return t
    raise AssertionError("no text with r = n found")


@pytest.mark.parametrize("pb", [4, 8])
def test_runs_at_the_extremes(pb):
    for t, r in ((_search_all_runs_text(), 8), (_t(b"A" * 300 + b"\x01"), 2)):
        sa = naive.suffix_array(t)
        heads, lens, brk = naive.rle(naive.bwt_from_sa(t, sa))
        assert len(heads) == r
        ssa, esa = naive.run_samples(sa, brk, len(t))
        got, A, d_text, d_sa = run_sa(t, pb)
        assert (got.astype(np.int64) == sa).all()
        g = run_runs(A, d_text, d_sa, len(t), pb, r)
        for a, b in zip(g, (heads, lens, ssa, esa)):
            assert (a == b).all()


@pytest.mark.parametrize("pb", [4, 8])
def test_a_text_that_breaks_the_rule_is_refused_and_the_output_untouched(pb):
    for t in (_t(b"ACGT\x01A"), _t(b"AC\x01GT\x01"), _t(b"ACGT"), _t(b"\x02ACGT\x03")):
        got, A, _, _ = run_sa(t, pb, want_rc=EARG)
        A.check_untouched("sa", [(0, len(t) * pb)])
    L = ra.lib()
    A = Arena(4096 + 8192, device="cuda")
    d = A.carve("x", 1024, align=256)
    assert L.rbg_suffix_array_dev(d.ptr, 0, d.ptr, pb, d.ptr, 1024, None) == EARG
    A.check_untouched("x", [(0, 1024)])
    assert L.rbg_sa_tmp_bytes(1 << 33, 4) == 0 and L.rbg_suffix_array_dev(d.ptr, 1 << 33, d.ptr, 4, d.ptr, 1024, None) == EARG


def test_two_million_symbols_against_the_torch_suffix_array():
    text, info = SP.make_text(100_000, 20, 0.001, 7, "cuda")
    assert info["n"] == 20 * 100_010 + 1
    want = SP.suffix_array(text)
    got = capi.suffix_array(text)
    assert got.dtype == torch.int32 and bool((got.to(torch.int64) == want).all())
    check_info(info["n"], 4)
    runs, ref = capi.text_runs(text, got), SP.index_inputs(text, want)
    assert runs["r"] == ref["r"] and all((runs[k] == ref[k]).all() for k in ("heads", "lens", "ssa", "esa"))
