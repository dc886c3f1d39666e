"""Exhaustive sweeps over a test-sized index, with their expected answers from text_ref.TextRef (the text and its suffix array; no
oracle): what tests/test_text_ref.py holds the oracle to on the CPU and tests/test_gpu_sweeps.py the device to.

    sweep A   every short pattern (all ACGT strings of lengths 1..9, absent ones included), every text window of lengths 10..24,
              windows of lengths 250..258 at every 7th start, every 12-symbol window with its first / middle / last symbol replaced
    sweep B   LF at every row: (i, i, c), (0, i, c), (i, n - 1, c) for every row i and (b - 1, b, c) for every run boundary b
    sweep C   locations: [i - 1, i] capped at 2 for every row (phi at every text position), the full range (one chain of n - 1
              steps), ranges of lengths 1..17 laid end to end under caps 2^64 - 1, 1, 8, 9 (stores at every alignment)

    sweep D   greedy seeds with and without samples, the longest seed and its locations: reads with a break at every offset (below)
    sweep E   toehold checkpoints and find_range_w_markers on the same reads and on the windows as the text has them; markers_at on
              every [i, i] and [i - 1, i]
    sweep F   marker seeds without an ftab and with K = 3, 10
    sweep G   lmems: every 24-symbol window and D1 cut to 24 symbols, one record per end position

The reads of sweeps D to F (SeedItems):
    D0  every 48-symbol window as the text has it, and the windows of D3 without their substitution (reads that OCCUR: checkpoints
        and find_range_w_markers answer nothing for the others)
    D1  every 48-symbol window with the symbol at offset start % 48 replaced by the ((start // 48) % 3 + 1)-th other base: a break at every
        offset of the read, so at every alignment to the k-mer steps and to every wsize
    D2  the same with N there (waves that mix the staged and the byte walk)
    D3  windows of 250..258 symbols at every D3_STRIDE-th start, one substitution at start % m (the edges of the staging cap)
    D4  for every D4_STRIDE-th start three 20-symbol windows from three distant starts, concatenated (lists of three and more seeds)
    D5  test_gpu_seeds_list's quirk reads, a read of one base, reads absent from their last symbol on, four windows that occur

An engine is anything with find_range / find_range_w_toehold / count (seqs, off), LF(lo, hi, c) and locs_at(lo, hi, k, max_hits):
rowbowt_amd.RowBowt as it is, the oracle through OracleEngine.  Sweeps D to G ask it for rowbowt_amd.RowBowt's seed and marker calls
(OracleSeedEngine puts the oracle and the per-read models behind them).  A mismatch raises one AssertionError that names the
configuration, the first differing item (its pattern, row or range), and how many items differ.
"""
import os
import time

import numpy as np

import text_ref as TR
from text_ref import MAXU, ACGT, acgt_patterns

SHORT_LENGTHS = tuple(range(1, 10))
WINDOW_LENGTHS = tuple(range(10, 25))
LONG_LENGTHS = tuple(range(250, 259))
LONG_STRIDE = 7
SUBST_LENGTH = 12
CHAIN_LENGTHS = tuple(range(1, 18))
CHAIN_CAPS = (MAXU, 1, 8, 9)


class Batch:
    """reads of one sub-sweep with what the text says about them"""

    def __init__(self, name, seqs, off, lo, hi, k):
        self.name, self.seqs, self.off, self.lo, self.hi, self.k = name, seqs, off, lo, hi, k

    def __len__(self):
        return len(self.off) - 1

    def describe(self, i):
        return "pattern %r" % self.seqs[int(self.off[i]):int(self.off[i + 1])].tobytes()


def _fixed(rows):
    """uint8 [N, m] -> (seqs, off)"""
    N, m = rows.shape
    return np.ascontiguousarray(rows).reshape(-1), np.arange(N + 1, dtype=np.uint64) * np.uint64(m)


def _join(parts):
    seqs = np.concatenate([s for s, _ in parts])
    lens = np.concatenate([np.diff(o) for _, o in parts])
    return seqs, np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)


def _windows(ref, lengths, stride):
    parts, lo, hi = [], [], []
    for m in lengths:
        starts = np.arange(0, ref.n - m + 1, stride, dtype=np.int64)     # (the last window ends in the terminator)
        parts.append(_fixed(ref.text[starts[:, None] + np.arange(m)]))
        wl, wh = ref.window_ranges(starts, m)
        lo.append(wl)
        hi.append(wh)
    seqs, off = _join(parts)
    lo, hi = np.concatenate(lo), np.concatenate(hi)
    return seqs, off, lo, hi, ref.toehold(lo, hi)


def short_patterns(ref):
    parts, lo, hi, present = [], [], [], {}
    for m in SHORT_LENGTHS:
        pats = acgt_patterns(m)
        parts.append(_fixed(pats))
        wl, wh = ref.ranges_of(pats)
        present[m] = int((wh >= wl).sum())
        lo.append(wl)
        hi.append(wh)
    seqs, off = _join(parts)
    lo, hi = np.concatenate(lo), np.concatenate(hi)
    b = Batch("A: every ACGT string of lengths 1..9", seqs, off, lo, hi, ref.toehold(lo, hi))
    b.present = present
    return b


def substituted_windows(ref):
    m = SUBST_LENGTH
    starts = np.arange(0, ref.n - m, dtype=np.int64)                      # (every window but the one that ends in the terminator)
    base = ref.text[starts[:, None] + np.arange(m)]
    rows = []
    for where in (0, m // 2, m - 1):
        for rot in (1, 2, 3):                                             # each of the three other bases
            w = base.copy()
            at = np.searchsorted(ACGT, w[:, where])
            acgt = (at < 4) & (ACGT[np.minimum(at, 3)] == w[:, where])
            w[:, where] = np.where(acgt, ACGT[(at + rot) & 3], w[:, where])
            rows.append(w[acgt])
    rows = np.concatenate(rows)
    lo, hi = ref.ranges_of(rows)
    seqs, off = _fixed(rows)
    return Batch("A: 12-symbol windows with the first, middle or last symbol replaced", seqs, off, lo, hi, ref.toehold(lo, hi))


def sweep_a(ref, short_only=False):
    out = [short_patterns(ref)]
    if not short_only:
        out.append(Batch("A: every text window of lengths 10..24", *_windows(ref, WINDOW_LENGTHS, 1)))
        out.append(Batch("A: windows of lengths 250..258 at every 7th start", *_windows(ref, LONG_LENGTHS, LONG_STRIDE)))
        out.append(substituted_windows(ref))
    return out


def sweep_b(ref, symbols):
    """-> lo, hi, c, want_lo, want_hi.  symbols: the bytes to ask for (present or not)"""
    n = ref.n
    rows = np.arange(n, dtype=np.int64)
    b = np.flatnonzero(ref.bwt[1:] != ref.bwt[:-1]) + 1                    # first rows of the runs after the first
    lo1 = np.concatenate((rows, np.zeros(n, np.int64), rows, b - 1))
    hi1 = np.concatenate((rows, rows, np.full(n, n - 1, np.int64), b))
    lo = np.tile(lo1, len(symbols))
    hi = np.tile(hi1, len(symbols))
    c = np.repeat(np.asarray(symbols, dtype=np.uint8), len(lo1))
    wlo, whi = ref.lf(lo, hi, c)
    return lo.astype(np.uint64), hi.astype(np.uint64), c, wlo, whi


class Ranges:
    def __init__(self, name, ref, lo, hi, max_hits):
        self.name, self.max_hits = name, max_hits
        self.lo, self.hi = lo.astype(np.uint64), hi.astype(np.uint64)
        self.k = ref.toehold(lo, hi)
        self.want_off, self.want_locs = ref.locs(lo, hi, max_hits)

    def describe(self, i):
        return "range [%d, %d] toehold %d max_hits %s" % (int(self.lo[i]), int(self.hi[i]), int(self.k[i]), "2^64-1" if self.max_hits == MAXU else self.max_hits)


def sweep_c(ref):
    n = ref.n
    rows = np.arange(1, n, dtype=np.int64)
    out = [Ranges("C(i): [i - 1, i] capped at 2, every row", ref, rows - 1, rows, 2),
           Ranges("C(ii): the full range", ref, np.zeros(1, np.int64), np.full(1, n - 1, np.int64), MAXU)]
    lens = np.resize(np.asarray(CHAIN_LENGTHS, dtype=np.int64), n)        # lengths 1..17 cycling; cut where the rows end
    ends = np.cumsum(lens)
    keep = ends <= n
    hi = ends[keep] - 1
    lo = hi - lens[keep] + 1
    if int(hi[-1]) < n - 1:
        lo, hi = np.append(lo, hi[-1] + 1), np.append(hi, n - 1)
    assert lo[0] == 0 and hi[-1] == n - 1 and (lo[1:] == hi[:-1] + 1).all()
    for cap in CHAIN_CAPS:
        out.append(Ranges("C(iii): ranges of lengths 1..17 end to end, max_hits %s" % ("2^64-1" if cap == MAXU else cap), ref, lo, hi, cap))
    return out


# ---- comparisons ---------------------------------------------------------------------------------------------------------------
def check_columns(cfg, what, got, want, describe):
    """got / want: tuples of equally long arrays; one message for the first differing item and the number of them"""
    bad = np.zeros(len(want[0]), dtype=bool)
    for g, w in zip(got, want):
        g = np.asarray(g)
        assert g.shape == w.shape, (cfg, what, g.shape, w.shape)
        bad |= g.astype(np.uint64) != w.astype(np.uint64)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: %s: %d of %d items differ; first at item %d, %s: got %s, the text says %s"
                             % (cfg, what, int(bad.sum()), len(bad), i, describe(i), tuple(int(g[i]) for g in got), tuple(int(w[i]) for w in want)))


def check_locs(cfg, r, got_off, got_locs):
    what = r.name
    check_columns(cfg, what + " (offsets)", (np.asarray(got_off)[1:],), (r.want_off[1:],), r.describe)
    got_locs = np.asarray(got_locs).astype(np.uint64)
    assert len(got_locs) == len(r.want_locs), (cfg, what, len(got_locs), len(r.want_locs))
    bad = np.flatnonzero(got_locs != r.want_locs)
    if len(bad):
        owner = np.searchsorted(r.want_off, bad, side="right") - 1
        i, at = int(owner[0]), int(bad[0])
        raise AssertionError("%s: %s: %d of %d ranges (%d of %d locations) differ; first at range %d, %s, location %d of it: got %d, the text says %d"
                             % (cfg, what, len(np.unique(owner)), len(r.lo), len(bad), len(got_locs), i, r.describe(i), at - int(r.want_off[i]),
                                int(got_locs[at]), int(r.want_locs[at])))


def run_sweep_a(cfg, engine, batches, forms=("find_range", "find_range_w_toehold", "count"), min_present_9=None):
    for b in batches:
        if "find_range_w_toehold" in forms:
            check_columns(cfg, b.name + " (find_range_w_toehold)", engine.find_range_w_toehold(b.seqs, b.off), (b.lo, b.hi, b.k), b.describe)
        if "find_range" in forms:
            check_columns(cfg, b.name + " (find_range)", engine.find_range(b.seqs, b.off), (b.lo, b.hi), b.describe)
        if "count" in forms:
            want = np.where(b.hi >= b.lo, b.hi - b.lo + np.uint64(1), np.uint64(0))
            got = np.asarray(engine.count(b.seqs, b.off))
            check_columns(cfg, b.name + " (count)", (got,), (want,), b.describe)
        if hasattr(b, "present"):
            # not vacuous: the patterns that occur, per length, as many as the text holds -- counted on what the engine answered
            lo, hi = engine.find_range(b.seqs, b.off)
            lens = np.diff(b.off).astype(np.int64)
            got = {m: int(((lens == m) & (hi >= lo)).sum()) for m in SHORT_LENGTHS}
            assert got == b.present, (cfg, got, b.present)
            if min_present_9 is not None:
                assert got[9] > min_present_9, (cfg, got)


def run_sweep_b(cfg, engine, B):
    lo, hi, c, wlo, whi = B
    check_columns(cfg, "B: LF at every row and run boundary", engine.LF(lo, hi, c), (wlo, whi),
                  lambda i: "LF((%d, %d), %r)" % (int(lo[i]), int(hi[i]), bytes([int(c[i])])))


def run_sweep_c(cfg, engine, C):
    for r in C:
        off, locs = engine.locs_at(r.lo, r.hi, r.k, r.max_hits)
        check_locs(cfg, r, off, locs)


class OracleEngine:
    """orc.Oracle behind the engine interface (batched, a few threads)"""

    def __init__(self, o, nthreads=None):
        self.o, self.nt = o, nthreads or min(8, os.cpu_count() or 1)

    def find_range(self, seqs, off):
        return self.o.find_range_batch(seqs, off, self.nt)

    def find_range_w_toehold(self, seqs, off):
        return self.o.find_range_w_toehold_batch(seqs, off, self.nt)

    def count(self, seqs, off):
        lo, hi = self.find_range(seqs, off)
        return np.where(hi >= lo, hi - lo + np.uint64(1), np.uint64(0))

    def LF(self, lo, hi, c):
        return self.o.LF_batch(lo, hi, c, self.nt)

    def locs_at(self, lo, hi, k, max_hits):
        return self.o.locs_at_batch(lo, hi, k, max_hits, self.nt)


# ---- the texts besides the synthetic pangenome -------------------------------------------------------------------------------------
def crowded_text():
    """the text of test_run_indexed_crowded_buckets (test_gpu_runs.py): 2 000 bases repeated 300 times, then 1 500 x (one of A, C, G, T + the
    same 14-mer + 10 random bases): consecutive rows whose BWT symbol changes at nearly every row beside buckets without a run"""
    rng = np.random.default_rng(7)
    block, x = ACGT[rng.integers(0, 4, 2000)], ACGT[rng.integers(0, 4, 14)]
    parts = [block] * 300 + [np.concatenate([ACGT[[i % 4]], x, ACGT[rng.integers(0, 4, 10)]]) for i in range(1500)]
    return np.concatenate(parts + [np.array([1], np.uint8)])


def alphabet_text(sigma=6, seed=1006):
    """a test_random_alphabets-style text (test_gpu_goldens.py): six mutated copies of 700 random symbols over `sigma` random bytes"""
    rng = np.random.default_rng(seed)
    alphabet = np.sort(rng.choice(np.arange(2, 256), size=sigma, replace=False)).astype(np.uint8)
    block = rng.choice(alphabet, size=700)
    pieces = []
    for _ in range(6):
        b = block.copy()
        b[rng.choice(len(b), size=12, replace=False)] = rng.choice(alphabet, size=12)
        pieces.append(b)
    return np.concatenate(pieces + [np.array([1], np.uint8)])


class Index:
    """a text with everything a load and the sweeps need: suffix array, run list, samples, TextRef"""

    def __init__(self, text, sa=None):
        import naive
        from text_ref import TextRef
        self.text = np.asarray(text, dtype=np.uint8)
        self.n = len(self.text)
        self.sa = naive.suffix_array(self.text) if sa is None else sa
        self.heads, self.lens, self.brk = naive.rle(naive.bwt_from_sa(self.text, self.sa))
        self.ssa, self.esa = naive.run_samples(self.sa, self.brk, self.n)
        self.ref = TextRef(self.text, self.sa)


# ---- sweeps D to G: seeds, checkpoints, marker windows, lmems ---------------------------------------------------------------------
READ_LENGTH = 48
LMEM_LENGTH = 24
D3_STRIDE = 7
D4_STRIDE = 5
CROWDED_MARKER_STRIDE = 4000   # (a site every two copies of the crowded text's block: 1 590 values, so that the walks that query the FULL range stay small)
MIN_LENGTHS = (0, 1, 10, 21)
MAX_HITS = (MAXU, 1, 3)
CHKPNT_WSIZES = (1, 5, 10, 19)
MARKER_TUPLES = ((10, MAXU), (7, 4), (19, 1000), (48, MAXU), (49, MAXU))
FTAB_KS = (0, 3, 10)
QUIRK_READS = [b"", b"N", b"NN", b"ACGTNNACGT", b"ACGNT", b"NACGT", b"ACGTN"]     # (test_gpu_seeds_list.QUIRK_READS)


def strided_markers(X, stride=40, wsize=10):
    """a marker array of SynthIndex.markers' shape for any text: a site at every `stride`-th position with allele (site / stride) % 3,
    tagged on the `wsize` positions up to it; rows through the ISA; neighbouring rows with equal value tuples merged into runs"""
    n = X.n
    sites = np.arange(stride - 1, n - 1, stride, dtype=np.int64)
    value = sites.astype(np.uint64) | (((sites // stride) % 3).astype(np.uint64) << np.uint64(60))
    pos = (sites[:, None] - np.arange(wsize)).reshape(-1)                  # (stride > wsize: one value per tagged position)
    assert stride > wsize
    rows = X.ref.isa[pos]
    order = np.argsort(rows)
    rows, vals = rows[order], np.repeat(value, wsize)[order]
    new = np.concatenate(([True], (rows[1:] != rows[:-1] + 1) | (vals[1:] != vals[:-1])))
    start = rows[new]
    end = rows[np.concatenate((np.flatnonzero(new)[1:] - 1, [len(rows) - 1]))]
    return start.astype(np.uint64), end.astype(np.uint64), np.arange(len(start) + 1, dtype=np.uint64), vals[new]


def _substituted(base, starts, m, with_n):
    w = base.copy()
    where = starts % m
    ar = np.arange(len(starts))
    at = np.searchsorted(ACGT, w[ar, where])
    assert (ACGT[at] == w[ar, where]).all()
    w[ar, where] = ord("N") if with_n else ACGT[(at + (starts // m) % 3 + 1) & 3]
    return w


class SeedItems:
    """the reads of sweeps D to F and of sweep G over one text; `every`: take every so-many-th read of D0 to D4 (1 on the device; the CPU
    leg against the per-read models strides, by a number coprime to 48 so that every break offset stays)"""

    def __init__(self, X, parts="01234", every=1, lmem_windows=True):
        ref, n, m = X.ref, X.n, READ_LENGTH
        text = X.text
        starts = np.arange(0, n - m, every, dtype=np.int64)               # (every window but the one that ends in the terminator)
        base = text[starts[:, None] + np.arange(m)]
        groups = []
        if "0" in parts:
            groups.append(("D0 window", _fixed(base), starts))
        if "1" in parts:
            groups.append(("D1 substituted window", _fixed(_substituted(base, starts, m, False)), starts))
        if "2" in parts:
            groups.append(("D2 window with N", _fixed(_substituted(base, starts, m, True)), starts))
        if "3" in parts:
            for ml in LONG_LENGTHS:
                s3 = np.arange(0, n - ml, D3_STRIDE * every, dtype=np.int64)
                b3 = text[s3[:, None] + np.arange(ml)]
                groups.append(("D0 window of %d" % ml, _fixed(b3), s3))
                groups.append(("D3 substituted window of %d" % ml, _fixed(_substituted(b3, s3, ml, False)), s3))
        if "4" in parts:
            s4 = np.arange(0, n - 21, D4_STRIDE * every, dtype=np.int64)
            cat = np.concatenate([text[((s4 + k * (n // 3)) % (n - 21))[:, None] + np.arange(20)] for k in range(3)], axis=1)
            groups.append(("D4 three windows", _fixed(cat), s4))
        t = text[:-1]
        d5 = QUIRK_READS + [t[7:8].tobytes(), t[100:147].tobytes() + b"N", t[200:247].tobytes() + bytes([ACGT[(np.searchsorted(ACGT, t[247]) + 1) & 3]]),
                           t[1960:2008].tobytes(), t[2500:2550].tobytes(), t[n - 60:n - 1].tobytes()]     # (reads that occur, (m - 1) % wsize both ways)
        d5 = [np.frombuffer(q, np.uint8) for q in d5]
        groups.append(("D5 quirk read", (np.concatenate(d5), np.concatenate(([0], np.cumsum([len(q) for q in d5]))).astype(np.uint64)), np.arange(len(d5))))
        self.seqs, self.off = _join([g[1] for g in groups])
        self.group_of = np.repeat(np.arange(len(groups)), [len(g[2]) for g in groups])
        self.names = [g[0] for g in groups]
        self.start = np.concatenate([g[2] for g in groups])
        self.break_at = np.where(np.isin(self.group_of, [j for j, g in enumerate(groups) if g[0].startswith(("D1", "D2"))]), self.start % m, -1)
        # sweep G
        ms = LMEM_LENGTH
        s = np.arange(0, n - ms, every, dtype=np.int64)
        plain = text[s[:, None] + np.arange(ms)]
        cut = _substituted(text[s[:, None] + np.arange(ms)], s, ms, False)
        self.lmem_seqs, self.lmem_off = _join(([_fixed(plain), _fixed(cut)] if lmem_windows else []) + [groups[-1][1]])

    def __len__(self):
        return len(self.off) - 1

    def describe(self, i):
        return "%s %d, read %r" % (self.names[int(self.group_of[i])], int(self.start[i]), self.seqs[int(self.off[i]):int(self.off[i + 1])].tobytes())

    def describe_lmem(self, i):
        return "read %r" % self.lmem_seqs[int(self.lmem_off[i]):int(self.lmem_off[i + 1])].tobytes()


class SeedSweeps:
    """the expected answers of sweeps D to G from the text (text_ref), made once per text; `seconds` is what that took"""

    def __init__(self, X, markers, items):
        t0 = time.perf_counter()
        ref = X.ref
        self.items, self.markers = items, markers
        self.mk = mk = TR.MarkerRef(*markers)
        I = items
        n = X.n
        # sweep D
        keys = [(ml, ws) for ml in MIN_LENGTHS for ws in (True, False)]

        def seeds(rows):
            V, E = TR.greedy_walk(ref, rows)
            return [TR.seeds_of_walk(V, E, ml, ws) for ml, ws in keys] + [TR.longest_of_walk(V, E, ml) for ml in MIN_LENGTHS]
        sets = TR.by_length(I.seqs, I.off, seeds)
        self.seeds = dict(zip(keys, sets[:len(keys)]))
        self.longest = {ml: s[1:] for ml, s in zip(MIN_LENGTHS, sets[len(keys):])}
        self.locs = {}
        for ml in MIN_LENGTHS:
            lo, hi, qs = self.longest[ml][:3]
            # (the same seeds as under a smaller min_length have the same locations: those arrays are kept once -- the crowded text has 3.6e8 per call at max_hits 2^64 - 1)
            same = next((p for p in MIN_LENGTHS[:MIN_LENGTHS.index(ml)] if all(np.array_equal(a, b) for a, b in zip(self.longest[p][:3], (lo, hi, qs)))), None)
            for mh in MAX_HITS:
                if same is not None:
                    self.locs[ml, mh] = self.locs[same, mh]
                    continue
                off, locs = ref.locs(lo, hi, mh)
                self.locs[ml, mh] = off, locs - np.repeat(qs, np.diff(off).astype(np.int64))
        # sweep E
        stats = {}

        def windows(rows):
            m = rows.shape[1]
            LO, HI, alive = TR.prefix_walk(ref, rows)
            out = [TR.chkpnts_of_walk(ref, m, LO, HI, alive, w) for w in CHKPNT_WSIZES]
            for w, mr in MARKER_TUPLES:
                a, b, st = TR.range_markers_of_walk(mk, m, LO, HI, alive, w, mr)
                out += [a, b]
                stats[w, mr] = tuple(x + y for x, y in zip(stats.get((w, mr), (0, 0, 0)), st))
                if m >= w and alive.any():
                    stats.setdefault("final", set()).add((w, (m - 1) % w == 0))
            return out
        sets = TR.by_length(I.seqs, I.off, windows)
        self.chkpnts = {w: s for w, s in zip(CHKPNT_WSIZES, sets)}
        rest = sets[len(CHKPNT_WSIZES):]
        self.range_markers = {t: (rest[2 * j][1], rest[2 * j][2], rest[2 * j + 1][0], rest[2 * j + 1][1]) for j, t in enumerate(MARKER_TUPLES)}
        self.marker_stats = stats
        rows = np.arange(n, dtype=np.int64)
        self.at_lo, self.at_hi = np.concatenate((rows, rows[1:] - 1)).astype(np.uint64), np.concatenate((rows, rows[1:])).astype(np.uint64)
        self.at = mk.at(self.at_lo, self.at_hi)
        # sweep F
        self.marker_seeds, self.ftab = {}, {}
        for K in FTAB_KS:
            hm = [0, 0, 0]

            def mseeds(rows, K=K, hm=hm):
                out, counts = TR.marker_seeds(ref, mk, rows, MARKER_TUPLES, K)
                for j in range(3):
                    hm[j] += counts[j]
                return out
            sets = TR.by_length(I.seqs, I.off, mseeds)
            for j, (w, mr) in enumerate(MARKER_TUPLES):
                self.marker_seeds[w, mr, K] = sets[2 * j] + sets[2 * j + 1]      # seed_off, lo, hi, qstart, qend, count, mk_off per read, values
            self.ftab[K] = tuple(hm)
        # sweep G
        self.lmems = {}
        for K in FTAB_KS:
            sets = TR.by_length(I.lmem_seqs, I.lmem_off, lambda rows, K=K: TR.marker_lmems(ref, mk, rows, MARKER_TUPLES, K), chunk=1 << 14)
            for j, (w, mr) in enumerate(MARKER_TUPLES):
                self.lmems[w, mr, K] = sets[2 * j] + sets[2 * j + 1]
        self.seconds = time.perf_counter() - t0

    def assert_not_vacuous(self, cfg, full=True, two_run_windows=True):
        """section 5 of the sweeps' plan, on the EXPECTED values; `full`: the unstrided items (the counts that need them all); two_run_windows:
        find_range_w_markers has queries answered from two or more runs (the synthetic pangenome has none under MARKER_TUPLES: DESIGN section 5)"""
        I = self.items
        off, lo, hi, qs, qe, ss = self.seeds[0, True]
        per = np.diff(off).astype(np.int64)
        broken = I.break_at >= 0
        assert set(I.break_at[broken & (per >= 2)].tolist()) == set(range(READ_LENGTH)), (cfg, "a break offset without a read of two seeds")
        many = int((np.diff(self.seeds[1, True][0]).astype(np.int64) >= 3).sum())
        assert "D4 three windows" not in I.names or many >= (1000 if full else 1), (cfg, many)      # (lists of three come from D4)
        zero = qe == qs
        stale = zero & (ss != np.uint64(MAXU)) & (hi - lo == np.uint64(len(self.at_lo) // 2))
        assert stale.any(), (cfg, "no zero-length seed with a stale ssamp")
        assert int(self.seeds[21, True][0][-1]) < int(self.seeds[10, True][0][-1]) < int(off[-1]), (cfg, "min_length drops nothing")
        answered, refused, two = self.marker_stats[7, 4]
        assert answered > 0 and refused > 0, (cfg, answered, refused)
        two_windows, two_seeds = sum(self.marker_stats[t][2] for t in MARKER_TUPLES), sum(self.ftab[K][2] for K in FTAB_KS)
        assert not full or two_seeds > 0, (cfg, "no marker-seed window whose query returns two runs' values")
        assert not (full and two_run_windows) or two_windows > 0, (cfg, "no find_range_w_markers query that returns two runs' values")
        hits, misses = self.ftab[10][:2]
        assert hits > 0 and misses > 0, (cfg, hits, misses)
        assert (np.diff(I.off).astype(np.int64) < 3).any() and (np.diff(I.off).astype(np.int64) < 10).any()
        finals = self.marker_stats["final"]
        assert {f for _, f in finals} == {True, False}, (cfg, finals)
        lens = np.diff(I.off).astype(np.int64)
        m1 = {(int(L) - 1) % w == 0 for w in CHKPNT_WSIZES for L in np.unique(lens[(np.diff(self.chkpnts[w][0]) > 0) & (lens >= 1)])}
        assert m1 == {True, False}, (cfg, m1)
        total = sum(len(v[3]) for v in self.range_markers.values()) + sum(len(v[7]) for v in self.marker_seeds.values()) + sum(len(v[7]) for v in self.lmems.values())
        assert total > 10 ** 4, (cfg, total)
        return dict(reads=len(I), seeds=int(off[-1]), three_or_more=many, stale=int(stale.sum()), markers=total, lmem_records=int(self.lmems[10, MAXU, 0][0][-1]),
                    two_run_window_queries=two_windows, two_run_seed_queries=two_seeds, ftab10_hits_misses=(hits, misses))


def check_ragged(cfg, what, got_off, got_vals, want_off, want_vals, describe):
    """offsets first, then values: the first differing read and how many differ"""
    check_columns(cfg, what + " (offsets)", (np.asarray(got_off)[1:],), (np.asarray(want_off)[1:],), describe)
    got_vals, want_vals = np.asarray(got_vals).astype(np.uint64, copy=False), np.asarray(want_vals).astype(np.uint64, copy=False)
    assert len(got_vals) == len(want_vals), (cfg, what, len(got_vals), len(want_vals))
    bad = np.flatnonzero(got_vals != want_vals)
    if len(bad):
        owner = np.searchsorted(np.asarray(want_off).astype(np.int64), bad, side="right") - 1
        i, at = int(owner[0]), int(bad[0])
        raise AssertionError("%s: %s: %d of %d items (%d of %d values) differ; first at item %d, %s, value %d of it: got %d, the text says %d"
                             % (cfg, what, len(np.unique(owner)), len(want_off) - 1, len(bad), len(want_vals), i, describe(i), at - int(want_off[i]),
                                int(got_vals[at]), int(want_vals[at])))


def _check_records(cfg, what, got, want, describe):
    """got / want: (offsets, column, ...): the offsets per read, then every column as values of the reads"""
    check_columns(cfg, what + " (records per read)", (np.asarray(got[0])[1:],), (want[0][1:],), describe)
    for j in range(1, len(want)):
        check_ragged(cfg, what + " (column %d)" % (j - 1), got[0], got[j], want[0], want[j], describe)


def _check_marker_records(cfg, what, got, want, off, describe):
    """got: (seed_off, seeds [S, 6], mk) of the host API; want: (seed_off, lo, hi, qstart, qend, count, mk_off per read, values)"""
    seed_off, seeds, mk = got
    cnt = seeds[:, 5] - seeds[:, 4]
    _check_records(cfg, what, (seed_off, seeds[:, 0], seeds[:, 1], seeds[:, 2], seeds[:, 3], cnt), want[:6], describe)
    assert len(seeds) == 0 or (int(seeds[0, 4]) == 0 and (seeds[1:, 4] == seeds[:-1, 5]).all()), (cfg, what, "marker ranges are not end to end")
    got_mk_off = np.concatenate(([0], np.cumsum(cnt.astype(np.int64))))[np.asarray(seed_off).astype(np.int64)]
    check_ragged(cfg, what + " (markers)", got_mk_off, mk, want[6], want[7], describe)


def run_sweep_d(cfg, eng, S, parts="DEFG"):
    """sweeps D to G on an engine with rowbowt_amd.RowBowt's seed and marker calls; -> per sweep the seconds, and under "compared" the number
    of EXPECTED records and marker / location values every one of which was compared (counted from the expected side: not a figure the engine
    can shrink)"""
    I = S.items
    took = {}
    n = {"D": 0, "E": 0, "F": 0, "G": 0}
    if "D" in parts or "d" in parts:
        n["D"] += sum(len(w[1]) for w in S.seeds.values())
    if "D" in parts:
        n["D"] += sum(len(w[0]) for w in S.longest.values()) + sum(len(w[1]) for w in S.locs.values())
    if "E" in parts:
        n["E"] += sum(len(w[1]) for w in S.chkpnts.values()) + sum(len(w[0]) + len(w[3]) for w in S.range_markers.values()) + len(S.at[1])
    if "F" in parts or "f" in parts:
        n["F"] += sum(len(w[1]) + len(w[7]) for w in S.marker_seeds.values())
    if "G" in parts:
        n["G"] += sum(len(w[1]) + len(w[7]) for w in S.lmems.values())
    took["compared"] = {k: v for k, v in n.items() if v}
    t0 = time.perf_counter()
    if "D" in parts or "d" in parts:                              # (d: the seed lists alone)
        for (ml, ws), want in S.seeds.items():
            _check_records(cfg, "D: get_seeds_greedy min_length %d %s" % (ml, "with samples" if ws else "without samples"),
                           eng.get_seeds_greedy(I.seqs, I.off, ml, ws), want, I.describe)
        for ml, want in S.longest.items() if "D" in parts else ():
            check_columns(cfg, "D: greedy_longest_seed min_length %d" % ml, eng.greedy_longest_seed(I.seqs, I.off, ml), want, I.describe)
            for mh in MAX_HITS:
                check_ragged(cfg, "D: find_locs_greedy_seeding min_length %d max_hits %s" % (ml, "2^64-1" if mh == MAXU else mh),
                             *eng.find_locs_greedy_seeding(I.seqs, I.off, ml, mh), *S.locs[ml, mh], I.describe)
        took["D"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    if "E" in parts:
        for w, want in S.chkpnts.items():
            _check_records(cfg, "E: find_range_w_toehold_chkpnts wsize %d" % w, eng.find_range_w_toehold_chkpnts(I.seqs, I.off, w), want, I.describe)
        for (w, mr), want in S.range_markers.items():
            what = "E: find_range_w_markers wsize %d max_range %s" % (w, "2^64-1" if mr == MAXU else mr)
            lo, hi, mk_off, mk = eng.find_range_w_markers(I.seqs, I.off, w, mr)
            check_columns(cfg, what, (lo, hi), want[:2], I.describe)
            check_ragged(cfg, what, mk_off, mk, want[2], want[3], I.describe)
        check_ragged(cfg, "E: markers_at [i, i] and [i - 1, i]", *eng.markers_at(S.at_lo, S.at_hi), *S.at,
                     lambda i: "range [%d, %d]" % (int(S.at_lo[i]), int(S.at_hi[i])))
        took["E"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    if "F" in parts or "f" in parts:
        for (w, mr, K), want in S.marker_seeds.items():
            what = "F: get_markers_greedy_seeding wsize %d max_range %s ftab_k %d" % (w, "2^64-1" if mr == MAXU else mr, K)
            _check_marker_records(cfg, what, eng.get_markers_greedy_seeding(I.seqs, I.off, w, mr, K), want, I.off, I.describe)
        took["F"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    if "G" in parts:
        for (w, mr, K), want in S.lmems.items():
            what = "G: get_markers_lmems wsize %d max_range %s ftab_k %d" % (w, "2^64-1" if mr == MAXU else mr, K)
            _check_marker_records(cfg, what, eng.get_markers_lmems(I.lmem_seqs, I.lmem_off, w, mr, K), want, I.lmem_off, I.describe_lmem)
        took["G"] = time.perf_counter() - t0
    return took


class OracleSeedEngine:
    """orc.Oracle, seeds_model and lmem_model behind rowbowt_amd.RowBowt's calls: one read at a time, in Python"""

    def __init__(self, o):
        self.o = o

    @staticmethod
    def _reads(seqs, off):
        b = seqs.tobytes()
        return [b[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]

    @staticmethod
    def _records(lists, ncol=5):
        off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64)
        flat = np.array([r[:ncol] for x in lists for r in x], dtype=np.uint64).reshape(-1, ncol)
        return (off,) + tuple(flat[:, c] for c in range(ncol))

    def get_seeds_greedy(self, seqs, off, min_length, w_sample=True):
        import seeds_model
        return self._records([seeds_model.seeds_greedy(self.o, q, min_length, w_sample) for q in self._reads(seqs, off)])

    def greedy_longest_seed(self, seqs, off, min_length):
        import seeds_model
        best = [seeds_model.longest_seed(seeds_model.seeds_greedy(self.o, q, min_length)) or (1, 0, 0, 0, 0) for q in self._reads(seqs, off)]
        return tuple(np.array(best, dtype=np.uint64).reshape(-1, 5).T)

    def find_locs_greedy_seeding(self, seqs, off, min_length, max_hits=MAXU):
        locs = [self.o.greedy_locate(q, min_length, max_hits)[0] for q in self._reads(seqs, off)]
        return np.concatenate(([0], np.cumsum([len(x) for x in locs]))).astype(np.uint64), np.array([v for x in locs for v in x], dtype=np.uint64)

    def find_range_w_toehold_chkpnts(self, seqs, off, wsize):
        import seeds_model
        return self._records([seeds_model.toehold_chkpnts(self.o, q, wsize) for q in self._reads(seqs, off)])

    def find_range_w_markers(self, seqs, off, wsize, max_range=MAXU):
        res = [self.o.find_range_w_markers(q, wsize, max_range) for q in self._reads(seqs, off)]
        return (np.array([r[0][0] for r in res], np.uint64), np.array([r[0][1] for r in res], np.uint64),
                np.concatenate(([0], np.cumsum([len(r[1]) for r in res]))).astype(np.uint64), np.array([v for r in res for v in r[1]], dtype=np.uint64))

    def markers_at(self, lo, hi):
        res = [self.o.markers_at(int(a), int(b)) for a, b in zip(lo, hi)]
        return np.concatenate(([0], np.cumsum([len(r) for r in res]))).astype(np.uint64), np.array([v for r in res for v in r], dtype=np.uint64)

    def _marker_records(self, lists):
        seed_off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64)
        recs = [r for x in lists for r in x]
        ends = np.cumsum([len(r[4]) for r in recs]).astype(np.uint64)
        seeds = np.zeros((len(recs), 6), np.uint64)
        if recs:
            seeds[:, :4] = np.array([r[:4] for r in recs], dtype=np.uint64)
            seeds[:, 5] = ends
            seeds[1:, 4] = ends[:-1]
        return seed_off, seeds, np.array([v for r in recs for v in r[4]], dtype=np.uint64)

    def get_markers_greedy_seeding(self, seqs, off, wsize, max_range=MAXU, ftab_k=0):
        return self._marker_records([self.o.markers_greedy_seeding(q, wsize, max_range, ftab_k) for q in self._reads(seqs, off)])

    def get_markers_lmems(self, seqs, off, wsize, max_range=MAXU, ftab_k=0):
        import lmem_model
        return self._marker_records([lmem_model.lmem_records(self.o, q, wsize, max_range, ftab_k) for q in self._reads(seqs, off)])
