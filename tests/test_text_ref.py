"""text_ref.TextRef (answers from the text and its suffix array alone) against naive.NaiveFM on sampled patterns and against the
oracle on EVERY item of the sweeps of tests/sweeps.py -- the same items tests/test_gpu_sweeps.py puts to the device.  A difference
between the oracle and the text is a finding about the oracle.  No GPU."""
import numpy as np
import pytest

import naive
import orc
import sweeps
import synth
from text_ref import ACGT, MAXU, acgt_patterns

TEXTS = ["synth", "random_a", "random_b", "crowded", "sigma6"]


def _make(name):
    if name == "synth":
        S = synth.SynthIndex()
        return sweeps.Index(S.text, S.fm.sa)
    if name == "random_a":      # near-random: almost every row its own run
        rng = np.random.default_rng(101)
        return sweeps.Index(np.concatenate([ACGT[rng.integers(0, 4, 1499)], np.array([1], np.uint8)]))
    if name == "random_b":      # a small pangenome with a skewed base composition (long runs of A)
        return sweeps.Index(synth.make_text(400, 5, 12, seed=4, pad=25)[0])
    if name == "crowded":
        return sweeps.Index(sweeps.crowded_text())
    return sweeps.Index(sweeps.alphabet_text())


_made = {}


def _index(name):
    """each text once per run (suffix sorting the crowded text takes a second or two)"""
    if name not in _made:
        _made[name] = _make(name)
    return _made[name]


def _fm(X):
    fm = naive.NaiveFM.__new__(naive.NaiveFM)      # (the suffix array is made already)
    fm.text, fm.n, fm.sa, fm.tb = X.text, X.n, X.sa, X.text.tobytes()
    return fm


@pytest.mark.parametrize("name", TEXTS)
def test_text_ref_equals_naive_fm_on_sampled_patterns(name):
    X = _index(name)
    ref, fm = X.ref, _fm(X)
    rng = np.random.default_rng(5)
    alphabet = ref.symbols[1:]
    checked = present = 0
    for m in (1, 2, 3, 5, 8, 9, 12, 17, 24):
        if ref.base ** m >= 2 ** 63:
            continue
        starts = rng.integers(0, X.n - m, 150)
        pats = X.text[starts[:, None] + np.arange(m)]
        pats[::3, rng.integers(0, m)] = alphabet[rng.integers(0, len(alphabet), len(pats[::3]))]     # a third of them with one symbol redrawn
        pats = np.concatenate([pats, alphabet[rng.integers(0, len(alphabet), (150, m))]])          # and as many random strings
        lo, hi = ref.ranges_of(pats)
        for j, p in enumerate(pats):
            want = fm.find_range(p.tobytes())
            assert (int(lo[j]), int(hi[j])) == want, (name, p.tobytes())
            if want[0] <= want[1]:
                present += 1
                if want[1] - want[0] < 5000:
                    assert ref.locs(lo[j:j + 1], hi[j:j + 1])[1].tolist() == fm.locs(*want)
                assert ref.locs(lo[j:j + 1], hi[j:j + 1], 3)[1].tolist() == X.sa[max(want[0], want[1] - 2):want[1] + 1][::-1].tolist()
        checked += len(pats)
    assert checked >= 2000 and present > checked // 3


@pytest.mark.parametrize("name", [t for t in TEXTS if t != "crowded"])     # (the crowded text takes the short patterns only: no windows in its sweep A)
def test_window_ranges_equal_keyed_ranges_and_naive_fm(name):
    """the two methods of text_ref (suffix keys + searchsorted; neighbouring rows' common prefixes) on every window both can answer, and
    the long windows against NaiveFM on a sample"""
    X = _index(name)
    ref = X.ref
    for m in (1, 2, 9, 10, 16, 24):
        if ref.base ** m >= 2 ** 63:
            continue
        starts = np.arange(0, X.n - m + 1)
        lo, hi = ref.window_ranges(starts, m)
        klo, khi = ref.ranges_of(X.text[starts[:, None] + np.arange(m)])
        assert (lo == klo).all() and (hi == khi).all(), (name, m)
    fm = _fm(X)
    rng = np.random.default_rng(6)
    for m in (25, 100, 250, 258, 300):
        starts = rng.integers(0, X.n - m + 1, 40)
        lo, hi = ref.window_ranges(starts, m)
        for j, s in enumerate(starts):
            assert (int(lo[j]), int(hi[j])) == fm.find_range(X.text[s:s + m].tobytes()), (name, m, int(s))


@pytest.mark.parametrize("name", [t for t in TEXTS if t != "sigma6"])      # (the texts over ACGT)
def test_lf_of_a_pattern_range_is_the_range_of_the_longer_pattern(name):
    """LF from cumulative counts against the ranges from suffix keys: LF(range(P), c) = range(cP) for every ACGT string P of lengths 1..6"""
    X = _index(name)
    ref = X.ref
    for m in range(1, 7):
        lo, hi = ref.pattern_ranges(m)
        live = hi >= lo
        longer = ref.pattern_ranges(m + 1)
        for ci, c in enumerate(ACGT):       # cP is pattern number ci * 4^m + (number of P)
            nlo, nhi = ref.lf(lo[live], hi[live], np.full(int(live.sum()), c, np.uint8))
            sel = ci * 4 ** m + np.flatnonzero(live)
            assert (nlo == longer[0][sel]).all() and (nhi == longer[1][sel]).all(), (name, m, chr(c))
            dead = ci * 4 ** m + np.flatnonzero(~live)
            assert (longer[0][dead] == 1).all() and (longer[1][dead] == 0).all()


def test_present_patterns_of_the_default_synthetic_index():
    """the sweep is not vacuous: of the 349 524 ACGT strings of lengths 1..9 these many occur in synth.SynthIndex()"""
    S = synth.SynthIndex()
    X = sweeps.Index(S.text, S.fm.sa)
    assert (X.n, len(X.heads)) == (18061, 2499)
    b = sweeps.short_patterns(X.ref)
    assert len(b) == 349524 and [b.present[m] for m in sweeps.SHORT_LENGTHS] == [4, 16, 64, 256, 978, 2198, 2937, 3184, 3274]
    assert len(acgt_patterns(3)) == 64 and acgt_patterns(3)[[0, 1, 4, 63]].tobytes() == b"AAAAACACATTT"


@pytest.mark.parametrize("name", TEXTS)
def test_oracle_equals_the_text_on_every_sweep_item(name):
    """oracle/rb_oracle.c (find_range_w_toehold_batch, LF, locs_at_batch) = text_ref on every item of sweeps A to C; the crowded text takes the
    short patterns of sweep A, the text over six other symbols sweeps B and C (with its own symbols and one it does not hold)"""
    X = _index(name)
    o = orc.Oracle.from_runs(X.heads, X.lens, X.ssa, X.esa)
    ref, E = X.ref, sweeps.OracleEngine(o)
    assert o.n == X.n and o.r == len(X.heads)
    if name != "sigma6":
        A = sweeps.sweep_a(ref, short_only=(name == "crowded"))
        sweeps.run_sweep_a(name, E, A, min_present_9=3000 if name in ("synth", "crowded") else None)
        symbols = list(b"ACGT\x01N")
    else:
        absent = next(c for c in range(2, 256) if ref.code[c] < 0)
        symbols = ref.symbols.tolist() + [absent]
    B = sweeps.sweep_b(ref, symbols)
    assert len(B[0]) == len(symbols) * (3 * X.n + len(X.heads) - 1)
    sweeps.run_sweep_b(name, E, B)
    C = sweeps.sweep_c(ref)
    sweeps.run_sweep_c(name, E, C)
    full = C[1]
    assert full.want_locs.tolist() == X.sa[::-1].tolist() and full.max_hits == MAXU     # the full range is the suffix array reversed
    o.close()


def test_a_wrong_answer_is_reported_with_its_item():
    """the message of a failing sweep: configuration, sub-sweep, how many items differ, the first one with its pattern / range"""
    X = _index("random_a")
    ref = X.ref

    class Off(sweeps.OracleEngine):
        def find_range_w_toehold(self, seqs, off):
            lo, hi, k = super().find_range_w_toehold(seqs, off)
            k[7] += np.uint64(1)
            return lo, hi, k

        def locs_at(self, lo, hi, k, max_hits):
            off, locs = super().locs_at(lo, hi, k, max_hits)
            locs[5] ^= np.uint64(1)
            return off, locs
    o = orc.Oracle.from_runs(X.heads, X.lens, X.ssa, X.esa)
    with pytest.raises(AssertionError, match=r"cfgX: A: every ACGT string.*1 of 349524 items differ; first at item 7, pattern b'AT'"):
        sweeps.run_sweep_a("cfgX", Off(o), [sweeps.short_patterns(ref)])
    with pytest.raises(AssertionError, match=r"cfgX: C\(i\).*1 of 1499 ranges \(1 of 2998 locations\) differ; first at range 2, range \[2, 3\] toehold \d+ max_hits 2, location 1 of it"):
        sweeps.run_sweep_c("cfgX", Off(o), sweeps.sweep_c(ref))
    o.close()
