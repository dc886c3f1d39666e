"""The answers of the query surface computed from the TEXT and its suffix array alone: pure numpy, no oracle, no run list.

A third line of defence next to oracle/rb_oracle.c (the C restatement of the reference) and naive.NaiveFM (binary search on
suffixes, one pattern at a time): everything here is vectorised, so that whole SWEEPS -- every short pattern, every text window,
every row, every text position -- get their expected answers in a second or so (tests/sweeps.py builds them).

Inputs: a text that ends in its unique smallest symbol (the terminator) and its suffix array (naive.suffix_array).

    ranges      inclusive (lo, hi) over the rows of the suffix array, (1, 0) for a pattern that does not occur: what RowBowt::LF /
                find_range return (rowbowt.hpp:74-88, :121-131).
    LF          LF((lo, hi), c) = (C[c] + occ(c, lo), C[c] + occ(c, hi + 1) - 1) from cumulative counts over the BWT
                (rowbowt.hpp:74-88); (1, 0) when c is not in the text or not in BWT[lo..hi].
    locations   of a non-empty [lo, hi]: SA[hi], SA[hi - 1], ..., SA[lo], cut at max_hits (ToeholdSA::locate_range,
                toehold_sa.hpp:37-49: phi(SA[i]) = SA[i - 1]).
    toehold     k = SA[hi] for a non-empty range, 0 for an empty one (LFData::clear, rowbowt.hpp:153-159).

Why k = SA[hi]: the reference keeps, per BWT run, y - 1 where y is the suffix array at the run's last row (n - 1 for y = 0:
toehold_sa.hpp:139-152).  find_range_w_toehold starts from the full range with k = samples_last[r - 1] + 1 = SA[n - 1]
(toehold_sa.hpp:97-99), i.e. k = SA[hi].  One step LF_w_loc (rowbowt.hpp:555-573) from (lo, hi, k = SA[hi]) with symbol c: the new
hi is LF(j) where j is the last row of [lo, hi] with BWT[j] = c, and SA[LF(j)] = SA[j] - 1.  If BWT[hi] = c then j = hi and the
step takes k - 1 = SA[hi] - 1; otherwise j ends a run of c (row j + 1 holds another symbol) and the step takes that run's
stored sample, SA[j] - 1.  Either way k = SA[new hi], by induction for every pattern.  The one exception is SA[j] = 0: there
BWT[j] is the terminator, so c is the terminator, and k becomes 2^64 - 1 (j = hi) or n - 1 (a run end).  A pattern holds the
terminator as its LAST symbol at most when it is a window of the text (the search is cyclic, a window is not), and its first
step then starts from hi = n - 1: the exception needs SA[n - 1] = 0, i.e. the whole text to be its own largest suffix.
`TextRef.toehold` therefore refuses a text with SA[n - 1] = 0 instead of modelling the wrap.
"""
import numpy as np

MAXU = 2**64 - 1
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
MAX_WINDOW = 300


def acgt_patterns(m):
    """all 4^m strings over ACGT of length m, in lexicographic order: uint8 [4^m, m]"""
    idx = np.arange(4 ** m, dtype=np.int64)
    shifts = 2 * np.arange(m - 1, -1, -1, dtype=np.int64)
    return ACGT[(idx[:, None] >> shifts[None, :]) & 3]


class TextRef:
    def __init__(self, text, sa):
        self.text = np.ascontiguousarray(text, dtype=np.uint8)
        self.sa = np.ascontiguousarray(sa, dtype=np.int64)
        self.n = n = len(self.text)
        assert n >= 2 and len(self.sa) == n and (np.bincount(self.sa, minlength=n) == 1).all(), "sa is no permutation of the text positions"
        term = int(self.text[n - 1])
        assert term == int(self.text.min()) and int((self.text == term).sum()) == 1, "the text must end in its unique smallest symbol"
        self.isa = np.empty(n, dtype=np.int64)
        self.isa[self.sa] = np.arange(n)
        self.symbols = np.unique(self.text)                       # ascending; symbols[0] is the terminator
        self.code = np.full(256, -1, dtype=np.int64)              # dense codes 1 .. sigma; 0 stands for "past the end of the text"
        self.code[self.symbols] = np.arange(1, len(self.symbols) + 1)
        self.base = len(self.symbols) + 1
        self.bwt = self.text[(self.sa - 1) % n]
        counts = np.bincount(self.text, minlength=256).astype(np.int64)
        self.C = np.concatenate(([0], np.cumsum(counts)))         # C[c] = symbols of the text smaller than c; C[c + 1] - C[c] = count of c
        self._occ = {}
        self._keys = {}
        self._lcp = None

    # ---- pattern ranges -----------------------------------------------------------------------------------------------------
    def keys(self, m):
        """every suffix keyed by its first m symbols (base sigma + 1, 0 past the end), in suffix-array order: ascending, or the
        suffix array is not one"""
        if m not in self._keys:
            assert self.base ** m < 2 ** 63, (self.base, m)
            codes = np.concatenate((self.code[self.text], np.zeros(m, dtype=np.int64)))
            key = np.zeros(self.n, dtype=np.int64)
            for j in range(m):
                key = key * self.base + codes[self.sa + j]
            assert (key[1:] >= key[:-1]).all(), "suffix keys do not ascend in suffix-array order"
            self._keys[m] = key
        return self._keys[m]

    def ranges_of(self, pats):
        """pats: uint8 [N, m], any bytes -> (lo, hi) uint64, (1, 0) where the pattern does not occur in the text (as a substring:
        a pattern with the terminator anywhere but at its end is refused, the index's search being cyclic)"""
        pats = np.asarray(pats, dtype=np.uint8)
        N, m = pats.shape
        codes = self.code[pats]
        assert not (pats[:, :-1] == self.symbols[0]).any(), "the terminator inside a pattern"
        known = (codes > 0).all(axis=1)
        key = np.zeros(N, dtype=np.int64)
        for j in range(m):
            key = key * self.base + np.maximum(codes[:, j], 0)
        keys = self.keys(m)
        lo = np.searchsorted(keys, key, side="left")
        hi = np.searchsorted(keys, key, side="right") - 1
        present = known & (hi >= lo)
        return np.where(present, lo, 1).astype(np.uint64), np.where(present, hi, 0).astype(np.uint64)

    def pattern_ranges(self, m):
        """(lo, hi) of all 4^m ACGT strings of length m, in the order of acgt_patterns(m)"""
        return self.ranges_of(acgt_patterns(m))

    def lcp(self):
        """lcp[i] = length of the common prefix of the suffixes at rows i - 1 and i, capped at MAX_WINDOW (lcp[0] = 0): by direct
        comparison, symbol by symbol"""
        if self._lcp is None:
            n, sa = self.n, self.sa
            a, b = sa[:-1].copy(), sa[1:].copy()
            rows = np.arange(1, n)
            lcp = np.zeros(n, dtype=np.int32)
            for _ in range(MAX_WINDOW):
                ok = (a < n) & (b < n)
                a, b, rows = a[ok], b[ok], rows[ok]
                eq = self.text[a] == self.text[b]
                a, b, rows = a[eq] + 1, b[eq] + 1, rows[eq]
                if len(rows) == 0:
                    break
                lcp[rows] += 1
            self._lcp = lcp
        return self._lcp

    def window_ranges(self, starts, m):
        """(lo, hi) of the text windows text[s : s + m] (s + m <= n, 1 <= m <= MAX_WINDOW): the rows around the window's own suffix
        whose neighbours share m symbols or more"""
        starts = np.asarray(starts, dtype=np.int64)
        assert 1 <= m <= MAX_WINDOW and (starts >= 0).all() and (starts + m <= self.n).all()
        brk = self.lcp() < m                                      # row i opens a new group of suffixes that share their first m symbols
        rows = np.arange(self.n)
        first = np.maximum.accumulate(np.where(brk, rows, 0))
        nxt = np.concatenate((brk[1:], [True]))                   # row i closes its group
        last = np.minimum.accumulate(np.where(nxt, rows, self.n - 1)[::-1])[::-1]
        row = self.isa[starts]
        return first[row].astype(np.uint64), last[row].astype(np.uint64)

    # ---- LF -----------------------------------------------------------------------------------------------------------------
    def occ(self, c):
        """occ[i] = number of c in BWT[0 .. i)"""
        if c not in self._occ:
            self._occ[c] = np.concatenate(([0], np.cumsum(self.bwt == c, dtype=np.int64)))
        return self._occ[c]

    def lf(self, lo, hi, c):
        """LF((lo, hi), c) for arrays of triples with lo <= hi < n -> (lo', hi') uint64"""
        lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
        c = np.asarray(c, dtype=np.uint8)
        assert (lo <= hi).all() and (hi < self.n).all() and (lo >= 0).all()
        nlo, nhi = np.ones(len(lo), dtype=np.int64), np.zeros(len(lo), dtype=np.int64)
        for sym in np.unique(c):
            sym = int(sym)
            if self.C[sym + 1] == self.C[sym]:
                continue                                          # not in the text
            sel = np.flatnonzero(c == sym)
            occ = self.occ(sym)
            before, upto = occ[lo[sel]], occ[hi[sel] + 1]
            some = upto > before
            nlo[sel] = np.where(some, self.C[sym] + before, 1)
            nhi[sel] = np.where(some, self.C[sym] + upto - 1, 0)
        return nlo.astype(np.uint64), nhi.astype(np.uint64)

    # ---- toeholds and locations ---------------------------------------------------------------------------------------------
    def toehold(self, lo, hi):
        """k of find_range_w_toehold: SA[hi], 0 for an empty range (the module's docstring has the derivation and the exception)"""
        assert self.sa[self.n - 1] != 0, "SA[n - 1] = 0: a window ending in the terminator would wrap its toehold below zero"
        lo, hi = np.asarray(lo).astype(np.int64), np.asarray(hi).astype(np.int64)
        return np.where(hi >= lo, self.sa[np.minimum(hi, self.n - 1)], 0).astype(np.uint64)

    def locs(self, lo, hi, max_hits=MAXU):
        """locs_at of N ranges -> (loc_off[N + 1], locs): SA[hi], SA[hi - 1], ... SA[lo] per range, at most max_hits of them"""
        lo, hi = np.asarray(lo).astype(np.int64), np.asarray(hi).astype(np.int64)
        occ = np.where(hi >= lo, hi - lo + 1, 0)
        if max_hits < MAXU:
            occ = np.minimum(occ, max_hits)
        off = np.concatenate(([0], np.cumsum(occ)))
        owner = np.repeat(np.arange(len(lo)), occ)
        rows = hi[owner] - (np.arange(int(off[-1])) - off[owner])
        return off.astype(np.uint64), self.sa[rows].astype(np.uint64)


# ---- seeds, checkpoints and marker windows from the text -----------------------------------------------------------------------
# Everything below steps TextRef.lf one symbol at a time over a whole batch of reads of one length (rows: uint8 [N, m]); a toehold
# is SA[hi] (the module's docstring), a marker answer is plain arithmetic on the marker arrays (MarkerRef.spans).  The rules, by the
# reference's line numbers (include/rowbowt.hpp):
#   get_seeds_greedy :191-215 / _w_sample :222-256   the walk starts at the read's right end from the full range; a failed step at q[p]
#       pushes (prev_range, p + 1, ei, pk) when ei - (p + 1) >= min_length (:200 / :237), then restarts from the full range with
#       ei = p (:205-207 / :243-246).  pk is the toehold of the LAST SUCCESSFUL step of the whole call (:249; 2^64 - 1 before any,
#       :232), so a zero-length seed carries the previous seed's.  The last record (prev_range, 0, ei, pk) is pushed always
#       without samples (:212) and when ei >= min_length with them (:252).  Without samples ssamp is left unset (:148-152): 0.
#   locate_from_longest_seed :669-677   the first seed of strictly greatest length; none or zero-length only: ((1, 0), 0, 0, 0).
#   find_locs_greedy_seeding :633-657   SA[hi], SA[hi - 1], ... of that seed, at most max_hits, each minus qstart.
#   find_range_w_toehold_chkpnts :575-606   no restart: a read that fails has no record.  After step i (0-based) a record
#       (range, m - i, window_ei, toehold) when window_ei - (m - i) >= wsize, then window_ei = m - i (:592-596): steps wsize,
#       2 wsize, ...; at the end (range, 0, m, toehold) when (m - 1) % wsize != 0 in 64-bit arithmetic (:599).
#   find_range_w_markers :292-339   m < wsize: nothing (:299-302).  The same steps and the same final test (:315, :328); each
#       query takes markers_at(range) when hi - lo + 1 <= max_range and PREPENDS them (:318-320, :331-333).
#   get_markers_greedy_seeding :406-482   update_mbuf appends (:437-441, markers_at does not clear :271-285).  With an ftab of
#       K-mers the walk starts at search_ftab(last K symbols) (:430-433): a hit is the K-mer's range and i = K, a miss the full
#       range and i = 0 (:757).  A failed step at q[p]: update(prev) when seed_ei - (p + 1) >= wsize (:445), fn(prev, p + 1,
#       seed_ei), mbuf cleared, seed_ei = window_ei = p (:448-453); with an ftab and p >= K the K-mer q[p - K : p] is looked up and
#       i += K whether it hits or misses -- a miss continues from the FULL range with K symbols skipped (:454-464: the test at
#       :459 holds for search_ftab's miss answer too).  A successful step to q[p]: update(range) and window_ei = p when
#       window_ei - p >= wsize (:469-472).  At the end update(range) when seed_ei - (m - i) >= wsize, fn(range, m - i, seed_ei)
#       (:478-481).  A read shorter than K (the reference throws in substr) starts like a miss, as the product documents.
#   get_markers_lmems :341-404   for every end e = m .. 1 the prefix q[0 : e] is walked once without restart; with an ftab and
#       e >= K it starts at search_ftab(q[e - K : e]) with i = K on a hit AND on a miss (:369-377).  Success at q[p]: update(range),
#       window_ei = p when window_ei - p >= wsize (:393-396).  Failure after i symbols: update(prev) when i >= wsize, fn(prev,
#       e - i, e) (:384-391).  The whole prefix: update(range) when e >= wsize, fn(range, 0, e) (:399-402).
def gather(vals, begin, count):
    """the concatenation of vals[begin[j] : begin[j] + count[j]]"""
    begin, count = np.asarray(begin, dtype=np.int64), np.asarray(count, dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(count)))
    owner = np.repeat(np.arange(len(count)), count)
    return vals[begin[owner] + np.arange(int(off[-1])) - off[owner]]


class MarkerRef:
    """MarkerArray::at_range on the arrays: the values of every run with start <= hi && end >= lo, in run order"""

    def __init__(self, run_start, run_end, mk_off, mk_vals):
        self.start, self.end = np.asarray(run_start).astype(np.int64), np.asarray(run_end).astype(np.int64)
        self.off, self.vals = np.asarray(mk_off).astype(np.int64), np.asarray(mk_vals).astype(np.uint64)
        assert (self.start <= self.end).all() and (self.start[1:] > self.end[:-1]).all() and len(self.off) == len(self.start) + 1

    def spans(self, lo, hi):
        """-> (begin, count) into vals, and the number of runs touched"""
        lo, hi = np.asarray(lo).astype(np.int64), np.asarray(hi).astype(np.int64)
        f = np.searchsorted(self.end, lo, side="left")
        l = np.searchsorted(self.start, hi, side="right")
        some = (l > f) & (hi >= lo)
        return self.off[f], np.where(some, self.off[l] - self.off[f], 0), np.where(some, l - f, 0)

    def at(self, lo, hi):
        b, c, _ = self.spans(lo, hi)
        return np.concatenate(([0], np.cumsum(c))).astype(np.uint64), gather(self.vals, b, c)


def by_length(seqs, off, fn, chunk=1 << 16):
    """fn(rows uint8 [N, m]) -> a list of ragged sets (counts[N], column, ...), records in read order; here over ragged reads: the
    reads of each length in chunks, the sets put back into the order of the reads -> per set (offsets[N + 1], column, ...)"""
    off = np.asarray(off).astype(np.int64)
    lens = np.diff(off)
    N = len(lens)
    parts = []
    for m in np.unique(lens):
        ids = np.flatnonzero(lens == m)
        for a in range(0, len(ids), chunk):
            sel = ids[a:a + chunk]
            parts.append((sel, fn(seqs[off[sel][:, None] + np.arange(int(m))].reshape(len(sel), int(m)))))
    out = []
    for s in range(len(parts[0][1])):
        counts = np.zeros(N, dtype=np.int64)
        for sel, sets in parts:
            counts[sel] = sets[s][0]
        order = np.argsort(np.concatenate([np.repeat(sel, sets[s][0]) for sel, sets in parts]), kind="stable")
        cols = tuple(np.concatenate([sets[s][1 + c] for _, sets in parts])[order] for c in range(len(parts[0][1][s]) - 1))
        out.append((np.concatenate(([0], np.cumsum(counts))).astype(np.uint64),) + cols)
    return out


def ftab_hits(ref, kmers):
    """search_ftab on the table build_ftab(K) makes: the ACGT-only K-mers that occur, with find_range's ranges -> hit, lo, hi"""
    lo, hi = ref.ranges_of(kmers)
    hit = np.isin(kmers, ACGT).all(axis=1) & (hi >= lo)
    return hit, lo.astype(np.int64), hi.astype(np.int64)


def greedy_walk(ref, rows):
    """one walk of get_seeds_greedy_w_sample over rows -> valid [N, m + 1] and (lo, hi, qstart, qend, ssamp) [5, N, m + 1]: column i what
    a failed step i would push, column m the last record; min_length has not been applied"""
    N, m = rows.shape
    n = ref.n
    lo, hi = np.zeros(N, np.int64), np.full(N, n - 1, np.int64)
    plo, phi = lo.copy(), hi.copy()
    ei = np.full(N, m, np.int64)
    pk = np.full(N, MAXU, np.uint64)
    V = np.zeros((N, m + 1), bool)
    E = np.zeros((5, N, m + 1), np.uint64)
    for i in range(m):
        nlo, nhi = ref.lf(lo, hi, rows[:, m - i - 1])
        fail = nhi < nlo
        V[:, i] = fail
        E[0, :, i], E[1, :, i], E[2, :, i], E[3, :, i], E[4, :, i] = plo, phi, m - i, ei, pk
        lo = np.where(fail, 0, nlo.astype(np.int64))
        hi = np.where(fail, n - 1, nhi.astype(np.int64))
        plo, phi = lo, hi
        pk = np.where(fail, pk, ref.sa[hi].astype(np.uint64))
        ei = np.where(fail, m - i - 1, ei)
    V[:, m] = True
    E[0, :, m], E[1, :, m], E[2, :, m], E[3, :, m], E[4, :, m] = plo, phi, 0, ei, pk
    return V, E


def seeds_of_walk(V, E, min_length, w_sample):
    """-> the ragged set (counts, lo, hi, qstart, qend, ssamp) of get_seeds_greedy[_w_sample]"""
    keep = V & ((E[3] - E[2]) >= np.uint64(min_length))
    if not w_sample:
        keep[:, -1] = True
    cols = [E[c][keep] for c in range(5)]
    if not w_sample:
        cols[4] = np.zeros_like(cols[4])
    return (keep.sum(axis=1),) + tuple(cols)


def longest_of_walk(V, E, min_length):
    """locate_from_longest_seed's choice among get_seeds_greedy_w_sample's list -> the set (ones, lo, hi, qstart, qend, ssamp)"""
    keep = V & ((E[3] - E[2]) >= np.uint64(min_length))
    length = np.where(keep, (E[3] - E[2]).astype(np.int64), 0)
    j = np.argmax(length, axis=1)                                  # (the first of the greatest)
    ar = np.arange(len(j))
    has = length[ar, j] > 0
    default = (1, 0, 0, 0, 0)
    return (np.ones(len(j), np.int64),) + tuple(np.where(has, E[c][ar, j], np.uint64(default[c])) for c in range(5))


def prefix_walk(ref, rows):
    """ranges of the suffixes q[m - i - 1:] after every step i -> LO, HI int64 [N, max(m, 1)] and alive[N] (the whole read occurs);
    an empty read keeps the full range in column 0"""
    N, m = rows.shape
    n = ref.n
    LO, HI = np.zeros((N, max(m, 1)), np.int64), np.full((N, max(m, 1)), n - 1, np.int64)
    alive = np.ones(N, bool)
    lo, hi = LO[:, 0].copy(), HI[:, 0].copy()
    for i in range(m):
        nlo, nhi = ref.lf(lo, hi, rows[:, m - i - 1])
        alive &= nhi >= nlo
        lo = np.where(alive, nlo.astype(np.int64), 0)
        hi = np.where(alive, nhi.astype(np.int64), n - 1)
        LO[:, i], HI[:, i] = lo, hi
    return LO, HI, alive


def _window_steps(m, wsize):
    """the steps after which a window closes, and whether the final record / query is made"""
    return np.arange(wsize, m, wsize, dtype=np.int64), ((m - 1) & MAXU) % wsize != 0


def chkpnts_of_walk(ref, m, LO, HI, alive, wsize):
    """find_range_w_toehold_chkpnts -> the set (counts, lo, hi, qstart, qend, ssamp)"""
    steps, final = _window_steps(m, wsize)
    cols = [np.concatenate((steps, [max(m, 1) - 1] if final else [])).astype(np.int64)]
    qs = np.concatenate((m - steps, [0] if final else []))
    qe = np.concatenate((m - steps + wsize, [m] if final else []))
    lo, hi = LO[alive][:, cols[0]], HI[alive][:, cols[0]]
    A, Q = lo.shape
    return (np.where(alive, Q, 0), lo.reshape(-1).astype(np.uint64), hi.reshape(-1).astype(np.uint64), np.tile(qs, A).astype(np.uint64),
            np.tile(qe, A).astype(np.uint64), ref.sa[hi.reshape(-1)].astype(np.uint64))


def range_markers_of_walk(mk, m, LO, HI, alive, wsize, max_range):
    """find_range_w_markers -> the sets (ones, lo, hi) and (counts, values); also (queries answered, refused, with >= 2 runs)"""
    N = len(alive)
    if m < wsize:
        return (np.ones(N, np.int64), np.ones(N, np.uint64), np.zeros(N, np.uint64)), (np.zeros(N, np.int64), mk.vals[:0]), (0, 0, 0)
    steps, final = _window_steps(m, wsize)
    q = np.concatenate((steps, [m - 1] if final else [])).astype(np.int64)[::-1]            # the last query's markers come first
    lo, hi = LO[:, q], HI[:, q]
    b, c, runs = mk.spans(lo, hi)
    asked = np.repeat(alive[:, None], len(q), axis=1)
    taken = asked & ((hi - lo + 1).astype(np.uint64) <= np.uint64(max_range))
    c = np.where(taken, c, 0)
    out_lo = np.where(alive, LO[:, m - 1], 1).astype(np.uint64)
    out_hi = np.where(alive, HI[:, m - 1], 0).astype(np.uint64)
    stats = (int(taken.sum()), int((asked & ~taken).sum()), int((taken & (runs >= 2)).sum()))
    return (np.ones(N, np.int64), out_lo, out_hi), (c.sum(axis=1), gather(mk.vals, b.reshape(-1), c.reshape(-1))), stats


class _Mbuf:
    """the marker buffers of one walk for several (wsize, max_range) at once: spans appended per record, in time order"""

    def __init__(self, mk, nrec, tuples):
        self.mk, self.tuples = mk, tuples
        self.count = [np.zeros(nrec, np.int64) for _ in tuples]
        self.ev = [[] for _ in tuples]
        self.time = 0
        self.two = 0                                              # queries answered from two or more runs

    def update(self, t, rec, lo, hi):
        """update_mbuf for the records `rec` (record = what the next fn() call reports) with the ranges lo, hi"""
        if not len(rec):
            return
        ok = (hi - lo + 1).astype(np.uint64) <= np.uint64(self.tuples[t][1])
        rec, lo, hi = rec[ok], lo[ok], hi[ok]
        b, c, runs = self.mk.spans(lo, hi)
        self.two += int((runs >= 2).sum())
        nz = c > 0
        self.ev[t].append((rec[nz], np.full(int(nz.sum()), self.time, np.int64), b[nz], c[nz]))
        np.add.at(self.count[t], rec, c)

    def values(self, t, nrec):
        """-> the values of all records in record order, each record's in time order"""
        if not self.ev[t]:
            return self.mk.vals[:0]
        rec, tm, b, c = (np.concatenate([e[j] for e in self.ev[t]]) for j in range(4))
        order = np.lexsort((tm, rec))
        return gather(self.mk.vals, b[order], c[order])


def marker_seeds(ref, mk, rows, tuples, K):
    """get_markers_greedy_seeding for every (wsize, max_range) of `tuples` in one walk -> per tuple the sets (seeds per read, lo, hi,
    qstart, qend, markers of the seed) and (markers per read, values); then (ftab hits, ftab misses, queries over two or more runs) of this walk"""
    N, m = rows.shape
    n, T = ref.n, len(tuples)
    ar = np.arange(N)
    l, h = np.zeros(N, np.int64), np.full(N, n - 1, np.int64)
    i = np.zeros(N, np.int64)
    hits = misses = 0
    if K and m >= K:
        hit, tl, th = ftab_hits(ref, rows[:, m - K:])
        l, h, i = np.where(hit, tl, l), np.where(hit, th, h), np.where(hit, K, 0)
        hits, misses = hits + int(hit.sum()), misses + int((~hit).sum())
    pl, ph = l.copy(), h.copy()
    seed_ei = np.full(N, m, np.int64)
    win = [np.full(N, m, np.int64) for _ in tuples]
    seq = np.zeros(N, np.int64)                                   # seeds emitted so far: a record is (read, seq)
    cap = m + 2
    mb = _Mbuf(mk, N * cap, tuples)
    S = [[] for _ in range(5)]

    def emit(sel, lo, hi, qs, qe):
        for lst, v in zip(S, (sel * cap + seq[sel], lo, hi, qs, qe)):
            lst.append(v)
        seq[sel] += 1

    while True:
        act = np.flatnonzero(i < m)
        if not len(act):
            break
        nl, nh = ref.lf(l[act], h[act], rows[act, m - i[act] - 1])
        fail = nh < nl
        F, G = act[fail], act[~fail]
        if len(F):
            p = m - i[F] - 1
            for t in range(T):
                sel = F[seed_ei[F] - (p + 1) >= tuples[t][0]]
                mb.update(t, sel * cap + seq[sel], pl[sel], ph[sel])
            emit(F, pl[F], ph[F], p + 1, seed_ei[F])
            seed_ei[F] = p
            for t in range(T):
                win[t][F] = p
            l[F], h[F] = 0, n - 1
            if K:
                R = p >= K
                FR = F[R]
                if len(FR):
                    hit, tl, th = ftab_hits(ref, rows[FR[:, None], (p[R] - K)[:, None] + np.arange(K)])
                    l[FR], h[FR] = np.where(hit, tl, 0), np.where(hit, th, n - 1)
                    i[FR] += K
                    hits, misses = hits + int(hit.sum()), misses + int((~hit).sum())
            pl[F], ph[F] = l[F], h[F]
        if len(G):
            l[G], h[G] = nl[~fail].astype(np.int64), nh[~fail].astype(np.int64)
            p = m - i[G] - 1
            for t in range(T):
                w = win[t][G] - p >= tuples[t][0]
                sel = G[w]
                mb.update(t, sel * cap + seq[sel], l[sel], h[sel])
                win[t][sel] = p[w]
            pl[G], ph[G] = l[G], h[G]
        i[act] += 1
        mb.time += 1
    for t in range(T):
        sel = ar[seed_ei - (m - i) >= tuples[t][0]]
        mb.update(t, sel * cap + seq[sel], l[sel], h[sel])
    emit(ar, l, h, m - i, seed_ei)
    rec, lo, hi, qs, qe = (np.concatenate(x) for x in S)
    order = np.argsort(rec, kind="stable")
    rec = rec[order]
    cols = tuple(x[order].astype(np.uint64) for x in (lo, hi, qs, qe))
    out = []
    for t in range(T):
        per_seed = mb.count[t][rec]
        per_read = np.bincount(rec // cap, weights=per_seed, minlength=N).astype(np.int64)
        out += [(seq.copy(),) + cols + (per_seed.astype(np.uint64),), (per_read, mb.values(t, N * cap))]
    return out, (hits, misses, mb.two)


def marker_lmems(ref, mk, rows, tuples, K):
    """get_markers_lmems for every (wsize, max_range) of `tuples` in one walk -> per tuple the sets (m records per read, lo, hi, qstart,
    qend, markers of the record) and (markers per read, values)"""
    N, m = rows.shape
    n, T = ref.n, len(tuples)
    R = np.repeat(np.arange(N), m)
    E = np.tile(np.arange(m, 0, -1, dtype=np.int64), N)           # record k of a read: the end position m - k
    nrec = N * m
    rec = np.arange(nrec)
    l, h = np.zeros(nrec, np.int64), np.full(nrec, n - 1, np.int64)
    i = np.zeros(nrec, np.int64)
    if K:
        sel = np.flatnonzero(E >= K)
        if len(sel):
            hit, tl, th = ftab_hits(ref, rows[R[sel][:, None], (E[sel] - K)[:, None] + np.arange(K)])
            l[sel], h[sel], i[sel] = np.where(hit, tl, 0), np.where(hit, th, n - 1), K
    win = [E.copy() for _ in tuples]
    done = np.zeros(nrec, bool)
    qs = np.zeros(nrec, np.int64)
    mb = _Mbuf(mk, nrec, tuples)
    while True:
        act = np.flatnonzero(~done & (i < E))
        if not len(act):
            break
        nl, nh = ref.lf(l[act], h[act], rows[R[act], E[act] - i[act] - 1])
        fail = nh < nl
        F, G = act[fail], act[~fail]
        for t in range(T):
            sel = F[i[F] >= tuples[t][0]]
            mb.update(t, sel, l[sel], h[sel])                     # (the range before the failed step)
        qs[F] = E[F] - i[F]
        done[F] = True
        l[G], h[G] = nl[~fail].astype(np.int64), nh[~fail].astype(np.int64)
        p = E[G] - i[G] - 1
        for t in range(T):
            w = win[t][G] - p >= tuples[t][0]
            sel = G[w]
            mb.update(t, sel, l[sel], h[sel])
            win[t][sel] = p[w]
        i[G] += 1
        mb.time += 1
    rest = rec[~done]
    for t in range(T):
        sel = rest[i[rest] >= tuples[t][0]]
        mb.update(t, sel, l[sel], h[sel])
    cols = tuple(x.astype(np.uint64) for x in (l, h, qs, E))
    out = []
    for t in range(T):
        per_read = mb.count[t].reshape(N, m).sum(axis=1) if m else np.zeros(N, np.int64)
        out += [(np.full(N, m, np.int64),) + cols + (mb.count[t].astype(np.uint64),), (per_read, mb.values(t, nrec))]
    return out
