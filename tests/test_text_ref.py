"""text_ref.TextRef (answers from the text and its suffix array alone) against naive.NaiveFM on sampled patterns and against the
oracle on EVERY item of the sweeps of tests/sweeps.py -- the same items tests/test_gpu_sweeps.py puts to the device.  A difference
between the oracle and the text is a finding about the oracle.  No GPU."""
import numpy as np
import pytest

import naive
import orc
import sweeps
import synth
import text_ref as TR
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


CPU_STRIDE = 97          # every 97th read of D0 to D4 and of the lmem windows on this leg (the per-read Python models): coprime to 48, so
                         # every break offset 0..47 stays (asserted below); every parameter tuple is kept.  The device leg takes every read.


def _synth_markers():
    S = synth.SynthIndex(L=4000, H=8, n_sites=60, seed=11)     # (the session fixture of the GPU files)
    return sweeps.Index(S.text, S.fm.sa), S.markers(10)


def test_oracle_and_models_equal_the_text_on_the_seed_sweeps():
    """orc.Oracle, seeds_model and lmem_model = text_ref on sweeps D to G, every CPU_STRIDE-th read: two restatements of the reference (the
    oracle's run-list arithmetic, the text's cumulative counts) agree before a device is asked"""
    X, mk = _synth_markers()
    I = sweeps.SeedItems(X, every=CPU_STRIDE)
    assert set(I.break_at[I.break_at >= 0].tolist()) == set(range(sweeps.READ_LENGTH))
    W = sweeps.SeedSweeps(X, mk, I)
    W.assert_not_vacuous("synth, every %d-th read" % CPU_STRIDE, full=False)
    assert len(W.marker_seeds) == len(W.lmems) == len(sweeps.MARKER_TUPLES) * len(sweeps.FTAB_KS) and len(W.seeds) == 2 * len(sweeps.MIN_LENGTHS)
    o = orc.Oracle.from_runs(X.heads, X.lens, X.ssa, X.esa)
    o.set_markers(*mk)
    sweeps.run_sweep_d("oracle", sweeps.OracleSeedEngine(o), W)
    o.close()


CROWDED_CPU_STRIDE = 977     # (the crowded text has 637 452 windows: every 977th, coprime to 48, 652 reads each of D1 and D2)


def test_oracle_and_models_equal_the_text_on_the_crowded_seed_sweeps():
    """the same on sweeps.crowded_text() with sweeps.strided_markers: D1, D2 and D5 (the lmems on D5), every CROWDED_CPU_STRIDE-th window"""
    X = _index("crowded")
    mk = sweeps.strided_markers(X, stride=sweeps.CROWDED_MARKER_STRIDE)
    I = sweeps.SeedItems(X, parts="12", every=CROWDED_CPU_STRIDE, lmem_windows=False)
    assert set(I.break_at[I.break_at >= 0].tolist()) == set(range(sweeps.READ_LENGTH))
    W = sweeps.SeedSweeps(X, mk, I)
    W.assert_not_vacuous("crowded, every %d-th read" % CROWDED_CPU_STRIDE, full=False)
    o = orc.Oracle.from_runs(X.heads, X.lens, X.ssa, X.esa)
    o.set_markers(*mk)
    took = sweeps.run_sweep_d("oracle", sweeps.OracleSeedEngine(o), W)
    assert took["compared"]["F"] > 10 ** 4, took
    o.close()


def test_every_seed_of_the_text_side_reference_is_a_maximal_match():
    """the greedy seeds of text_ref.greedy_walk checked by something that is not its loop, on every read of sweep D: a seed q[s:e] with e > s has
    exactly the range of that string (window_ranges at one of its occurrences, which spells it), q[s-1:e] does not occur (ranges_of up to 23
    symbols; above, no suffix of the range is preceded by q[s-1]), and the next seed ends at s - 1.  Then section 5's conditions on all reads."""
    X, mk = _synth_markers()
    ref = X.ref
    I = sweeps.SeedItems(X)
    sets = TR.by_length(I.seqs, I.off, lambda rows: [TR.seeds_of_walk(*TR.greedy_walk(ref, rows), 0, True)])
    off, lo, hi, qs, qe, ss = (a.astype(np.int64) if j else a for j, a in enumerate(sets[0]))
    owner = np.repeat(np.arange(len(I)), np.diff(off).astype(np.int64))
    first = np.concatenate(([True], owner[1:] != owner[:-1]))
    roff = I.off.astype(np.int64)
    assert (qe[first] == np.diff(roff)[owner[first]]).all() and (qe[~first] == qs[:-1][~first[1:]] - 1).all() and (qs[np.concatenate((first[1:], [True]))] == 0).all()
    length = qe - qs
    checked = 0
    for m in np.unique(length[length > 0]):
        sel = np.flatnonzero(length == m)
        at = X.sa[lo[sel]]
        spelled = I.seqs[(roff[owner[sel]] + qs[sel])[:, None] + np.arange(m)]
        assert (X.text[at[:, None] + np.arange(m)] == spelled).all(), m
        wl, wh = ref.window_ranges(at, int(m))                  # (asserts m <= text_ref.MAX_WINDOW: no read of the sweeps is longer)
        assert (wl.astype(np.int64) == lo[sel]).all() and (wh.astype(np.int64) == hi[sel]).all(), m
        inner = sel[qs[sel] > 0]
        before = I.seqs[roff[owner[inner]] + qs[inner] - 1]
        if m < 23:
            el, eh = ref.ranges_of(np.concatenate((before[:, None], I.seqs[(roff[owner[inner]] + qs[inner])[:, None] + np.arange(m)]), axis=1))
            assert (eh < el).all(), m
        else:
            cnt = hi[inner] - lo[inner] + 1
            rows = TR.gather(np.arange(X.n), lo[inner], cnt)
            assert (ref.bwt[rows] != np.repeat(before, cnt)).all(), m
        checked += len(sel)
    assert checked > 150000
    zero = length == 0
    assert zero.any() and (lo[zero] == 0).all() and (hi[zero] == X.n - 1).all()


def test_the_seed_sweeps_are_not_vacuous_on_the_whole_text():
    """section 5 on the expected values of every read (what the device leg compares), and the time to build them beside sweeps A to C's"""
    import time
    X, mk = _synth_markers()
    t0 = time.perf_counter()
    sweeps.sweep_a(X.ref), sweeps.sweep_b(X.ref, list(b"ACGT\x01N")), sweeps.sweep_c(X.ref)
    abc = time.perf_counter() - t0
    W = sweeps.SeedSweeps(X, mk, sweeps.SeedItems(X))
    print("expected values: sweeps A to C %.1f s, sweeps D to G %.1f s; %s" % (abc, W.seconds, W.assert_not_vacuous("synth", two_run_windows=False)))


def test_strided_markers_are_the_arrays_of_the_text():
    """sweeps.strided_markers against a plain loop over the tagged positions"""
    X = _index("random_b")
    ms, me, mo, mv = sweeps.strided_markers(X, stride=40, wsize=10)
    want = {}
    for site in range(39, X.n - 1, 40):
        for d in range(10):
            want[int(X.ref.isa[site - d])] = site | (((site // 40) % 3) << 60)
    got = {}
    for a, b, v in zip(ms.tolist(), me.tolist(), mv.tolist()):
        for row in range(a, b + 1):
            got[row] = v
    assert got == want and (np.diff(mo) == 1).all() and len(ms) < len(want)
    merged = [(a, b) for a, b in zip(ms.tolist(), me.tolist()) if b > a]
    assert merged and all(mv[j] != mv[j + 1] or me[j] + 1 < ms[j + 1] for j in range(len(ms) - 1))


def test_one_wrong_value_fails_the_seed_sweeps_and_names_its_read():
    """run_sweep_d bites: ONE changed ssamp, ONE changed marker value, ONE changed lmem qstart behind the oracle engine each raise, with the
    configuration, the sweep, the count of differing items and the read; the untouched engine passes (the test above)"""
    X, mk = _synth_markers()
    W = sweeps.SeedSweeps(X, mk, sweeps.SeedItems(X, every=CPU_STRIDE * 5))
    o = orc.Oracle.from_runs(X.heads, X.lens, X.ssa, X.esa)
    o.set_markers(*mk)

    class Ssamp(sweeps.OracleSeedEngine):
        def get_seeds_greedy(self, seqs, off, min_length, w_sample=True):
            res = super().get_seeds_greedy(seqs, off, min_length, w_sample)
            if w_sample and min_length == 10:
                res[5][3] ^= np.uint64(1)
            return res

    class Marker(sweeps.OracleSeedEngine):
        def get_markers_greedy_seeding(self, seqs, off, wsize, max_range=MAXU, ftab_k=0):
            so, seeds, vals = super().get_markers_greedy_seeding(seqs, off, wsize, max_range, ftab_k)
            if (wsize, ftab_k) == (19, 3):
                assert len(vals) > 9
                vals[9] ^= np.uint64(1)
            return so, seeds, vals

    class Lmem(sweeps.OracleSeedEngine):
        def get_markers_lmems(self, seqs, off, wsize, max_range=MAXU, ftab_k=0):
            so, seeds, vals = super().get_markers_lmems(seqs, off, wsize, max_range, ftab_k)
            if (wsize, max_range, ftab_k) == (7, 4, 10):
                seeds[30, 2] += np.uint64(1)
            return so, seeds, vals
    with pytest.raises(AssertionError, match=r"cfgX: D: get_seeds_greedy min_length 10 with samples \(column 4\).*1 of \d+ items \(1 of \d+ values\) differ; first at item \d+, D"):
        sweeps.run_sweep_d("cfgX", Ssamp(o), W, parts="d")
    with pytest.raises(AssertionError, match=r"cfgX: F: get_markers_greedy_seeding wsize 19 max_range 1000 ftab_k 3 \(markers\).*\(1 of \d+ values\) differ; first at item \d+, D"):
        sweeps.run_sweep_d("cfgX", Marker(o), W, parts="f")
    with pytest.raises(AssertionError, match=r"cfgX: G: get_markers_lmems wsize 7 max_range 4 ftab_k 10 \(column 2\).*\(1 of \d+ values\) differ; first at item 1, read b'"):
        sweeps.run_sweep_d("cfgX", Lmem(o), W, parts="G")
    took = sweeps.run_sweep_d("cfgX", sweeps.OracleSeedEngine(o), W)
    assert set(took["compared"]) == set("DEFG") and all(v > 1000 for v in took["compared"].values()), took
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
