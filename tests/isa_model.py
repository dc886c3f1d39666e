"""Test infrastructure: the ISA sample of rowbowt_amd/csrc/rbg_isa.hpp -- builder, directory, lookup, the row of a text position and the text of an interval
(include/rbg.h: rbg_extract_prepare, rbg_isa_dev, rbg_extract_dev) -- in Python integers over the runs of a BWT (heads, lens) and the raw run samples (ssa,
esa: the suffix array at the first / last row of every run), on top of fl_model.FL.  Nothing here looks at the library.

    samples   {tpos, row} with tpos = SA[row]: (1) the last row of every run, tpos = esa[i]; (2) every row whose BWT symbol is not one of A C G T and that does
              not end its run, its SA from the run's last row downwards by phi (toehold_sa.hpp:56-72 over the run-start samples).  Sorted by tpos.
    dir[b]    the index of the largest sample with tpos <= b << shift, shift = max(0, floor(log2(n / S))), (n >> shift) + 2 entries
    lookup(p) the sample with the largest tpos <= p;  isa(p) = p - tpos FL steps from its row
    extract   FL steps from isa(p), each giving the row's F byte, up to the first row without a base: (len bytes -- the bases, then zeros --, got)
"""
import bisect
import functools

import numpy as np

import fl_model as FM
import naive

ACGT = b"ACGT"
LENS = (0, 1, 2, 15, 16, 17, 33, 70)      # the interval lengths every position is read with


class ISA:
    def __init__(self, heads, lens, ssa, esa, second_kind=True):
        heads, lens = [int(h) for h in heads], [int(l) for l in lens]
        ssa, esa = [int(v) for v in ssa], [int(v) for v in esa]
        self.fl = FM.FL(heads, lens)
        self.n = n = sum(lens)
        R = len(heads)
        start = [0] * (R + 1)
        for i, l in enumerate(lens):
            start[i + 1] = start[i] + l
        # the toehold's arrays: SA - 1 at the runs' ends; the runs' starts (SA - 1) in text order with the end sample of the run before
        samples_last = [(v - 1) % n for v in esa]
        order = sorted(range(R), key=lambda i: (ssa[i] - 1) % n)
        pred_pos = [(ssa[i] - 1) % n for i in order]
        phi_base = [samples_last[i - 1] if i else 0 for i in order]

        def phi(i):
            below = bisect.bisect_left(pred_pos, i)
            jr = below - 1 if below else R - 1
            j = pred_pos[jr]
            return (phi_base[jr] + (i - j if j < i else i + 1)) % n

        pairs = [((samples_last[i] + 1) % n, start[i + 1] - 1) for i in range(R)]
        self.second_kind = 0
        self.longest_other_run = 0
        for i in range(R):
            if heads[i] in ACGT:
                continue
            self.longest_other_run = max(self.longest_other_run, lens[i])
            sa = (samples_last[i] + 1) % n
            for row in range(start[i + 1] - 1, start[i], -1):
                sa = phi(sa)
                if second_kind:
                    pairs.append((sa, row - 1))
                    self.second_kind += 1
        pairs.sort()
        self.tpos = [p for p, _ in pairs]
        self.row = [r for _, r in pairs]
        assert self.tpos[0] == 0 and len(set(self.tpos)) == len(pairs)
        self.samples = S = len(pairs)
        self.shift = 0
        while (S << (self.shift + 1)) <= n:
            self.shift += 1
        self.dir_entries = (n >> self.shift) + 2
        self.dir = [bisect.bisect_right(self.tpos, b << self.shift) - 1 for b in range(self.dir_entries)]
        self.max_gap = max(b - a for a, b in zip(self.tpos, self.tpos[1:] + [n]))

    def bytes(self, pos_bytes):
        return self.samples * 2 * pos_bytes + self.dir_entries * pos_bytes

    def lookup(self, p):
        """(tpos, row) of the sample before p, through the directory: a bisection within [dir[b], dir[b + 1]]"""
        assert 0 <= p < self.n
        b = p >> self.shift
        a, z = self.dir[b], self.dir[b + 1]
        assert self.tpos[a] <= p and (z + 1 == self.samples or self.tpos[z + 1] > p)
        while a < z:
            mid = a + ((z - a + 1) >> 1)
            if self.tpos[mid] <= p:
                a = mid
            else:
                z = mid - 1
        return self.tpos[a], self.row[a]

    def isa(self, p):
        """the row of the suffix at p; None when the walk-in meets a row without a base"""
        q, row = self.lookup(p)
        for _ in range(p - q):
            c, row = self.fl.step(row)
            if c == 0:
                return None
        return row

    def extract_from(self, row, length):
        """(length bytes: the bases from `row` on, then zeros; got)"""
        out = bytearray()
        while len(out) < length:
            c, row = self.fl.step(row)
            if c == 0:
                break
            out.append(c)
        got = len(out)
        return bytes(out) + bytes(length - got), got

    def extract(self, p, length):
        return self.extract_from(self.isa(p), length)


def expected(text, p, length):
    """what extract gives by the text alone: text[p:] up to the first byte that is not a base, at most `length`, then zeros"""
    got = 0
    while got < length and p + got < len(text) and text[p + got] in ACGT:
        got += 1
    return bytes(text[p:p + got]) + bytes(length - got), got


class Text:
    """a text that ends in its terminator, with everything the tests read off it: sa, isa, the runs of its BWT and their samples"""

    def __init__(self, text, doc_names=None, doc_starts=None):
        self.text = np.frombuffer(bytes(text), dtype=np.uint8).copy()
        self.tb = bytes(text)
        self.n = len(self.tb)
        self.sa = naive.suffix_array(self.text)
        self.isa = np.empty(self.n, dtype=np.int64)
        self.isa[self.sa] = np.arange(self.n)
        self.bwt = naive.bwt_from_sa(self.text, self.sa)
        self.heads, self.lens, self.brk = naive.rle(self.bwt)
        self.ssa, self.esa = naive.run_samples(self.sa, self.brk, self.n)
        self.doc_names, self.doc_starts = doc_names, doc_starts

    def model(self, second_kind=True):
        return ISA(self.heads, self.lens, self.ssa, self.esa, second_kind)


@functools.lru_cache(maxsize=None)
def synth_text():
    """SynthIndex(L=400, H=5, n_sites=12, seed=41): n = 2051, one byte that is no base (the terminator)"""
    from synth import SynthIndex
    S = SynthIndex(L=400, H=5, n_sites=12, seed=41)
    T = Text(S.text.tobytes(), S.doc_names, S.doc_starts)
    assert T.n == 2051 and sum(c not in ACGT for c in T.tb) == 1
    return T


@functools.lru_cache(maxsize=None)
def hand_text():
    """three documents separated by '#': the second starts with N and holds a run of five N, the third is a near copy of the first with single N"""
    rng = np.random.default_rng(97)
    base = bytes(rng.choice(np.frombuffer(ACGT, np.uint8), 160).tolist())
    d0 = base
    d1 = b"N" + base[10:90] + b"NNNNN" + base[60:130] + b"A"
    d2 = bytearray(base[:150])
    d2[40], d2[41], d2[97] = ord("N"), ord("G") if base[41] != ord("G") else ord("C"), ord("N")
    text = d0 + b"#" + d1 + b"#" + bytes(d2) + b"\x01"
    starts = [0, len(d0) + 1, len(d0) + 1 + len(d1) + 1]
    return Text(text, ["d0", "d1", "d2"], starts)
