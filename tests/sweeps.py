"""Exhaustive sweeps over a test-sized index, with their expected answers from text_ref.TextRef (the text and its suffix array; no
oracle): what tests/test_text_ref.py holds the oracle to on the CPU and tests/test_gpu_sweeps.py the device to.

    sweep A   every short pattern (all ACGT strings of lengths 1..9, absent ones included), every text window of lengths 10..24,
              windows of lengths 250..258 at every 7th start, every 12-symbol window with its first / middle / last symbol replaced
    sweep B   LF at every row: (i, i, c), (0, i, c), (i, n - 1, c) for every row i and (b - 1, b, c) for every run boundary b
    sweep C   locations: [i - 1, i] capped at 2 for every row (phi at every text position), the full range (one chain of n - 1
              steps), ranges of lengths 1..17 laid end to end under caps 2^64 - 1, 1, 8, 9 (stores at every alignment)

An engine is anything with find_range / find_range_w_toehold / count (seqs, off), LF(lo, hi, c) and locs_at(lo, hi, k, max_hits):
rowbowt_amd.RowBowt as it is, the oracle through OracleEngine.  A mismatch raises one AssertionError that names the configuration,
the first differing item (its pattern, row or range), and how many items differ.
"""
import os

import numpy as np

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
