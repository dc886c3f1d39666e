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
