"""Test infrastructure: FL over the run arrays of a BWT in Python integers, the right walk of rbg_extend_right_dev and the lines of rbg_align_sam_extend_both
(include/rbg.h; the rules: rowbowt_amd/csrc/rbg_fl.hpp and rbg_sam.hpp), on top of sam_extend_model.py.  Nothing here looks at the library.

    FL(i) = select_c(BWT, i - F[c]): c = the byte whose F interval holds row i; the (i - F[c])-th c of the BWT (counted from 0) sits in the c-run j with
    cum[j] <= i - F[c] < cum[j + 1], at BWT position start[j] + (i - F[c] - cum[j]).
"""
import bisect

import sam_extend_model as XM
import sam_model as SAM

ACGT = b"ACGT"
NONE = 2**64 - 1


class FL:
    def __init__(self, heads, lens):
        """heads[R] (bytes), lens[R]: the runs of the BWT"""
        self.n = 0
        self.cum = {c: [] for c in ACGT}          # per base: the number of c before each of its runs
        self.pos = {c: [] for c in ACGT}          # ... and the BWT position where the run starts
        counts = [0] * 257
        for h, l in zip((int(x) for x in heads), (int(x) for x in lens)):
            if h in self.cum:
                self.cum[h].append(counts[h])
                self.pos[h].append(self.n)
            counts[h] += l
            self.n += l
        self.count = counts
        self.F = [0] * 257
        for c in range(256):
            self.F[c + 1] = self.F[c] + counts[c]

    def runs(self, c):
        return len(self.cum[c])

    def shift(self, c):
        """max(0, floor(log2(n_c / runs_c))): the largest s with runs_c << s <= n_c"""
        s = 0
        while self.runs(c) and (self.runs(c) << (s + 1)) <= self.count[c]:
            s += 1
        return s

    def bytes(self, pos_bytes):
        """per base present (runs + 1) * 2 * pos_bytes + ((n_c >> shift) + 2) * pos_bytes"""
        return sum((self.runs(c) + 1) * 2 * pos_bytes + ((self.count[c] >> self.shift(c)) + 2) * pos_bytes for c in ACGT if self.runs(c))

    def step(self, row):
        """(sym, FL(row)); (0, 2^64 - 1) when the row's F byte is not one of A C G T"""
        assert 0 <= row < self.n
        for c in ACGT:
            if self.F[c] <= row < self.F[c] + self.count[c]:
                k = row - self.F[c]
                j = bisect.bisect_right(self.cum[c], k) - 1
                return c, self.pos[c][j] + (k - self.cum[c][j])
        return 0, NONE


def walk_right(s, b, L, K, base_at):
    """sam_extend_model.walk_bases with x = s[b + t]: base_at(t) = the reference byte t positions right of the seed's end"""
    rs = bytes(s)[::-1]                             # rs[(len - b) - 1 - t] = s[b + t]
    return XM.walk_bases(rs, len(rs) - b, L, K, base_at)


def extend_right(fl, s, b, row, skip, limit, K):
    """the rule over the FL model: `skip` steps without comparing (no base on the way: the zero record), then the walk"""
    r = row
    for _ in range(skip):
        c, r = fl.step(r)
        if c == 0:
            return dict(ext=0, nm=0, score=0, steps=0, mis=[], why="skip")
    state = {"r": r, "t": -1}

    def base_at(t):
        assert t == state["t"] + 1
        if t > 0:
            state["r"] = state["next"]
        state["t"] = t
        c, state["next"] = fl.step(state["r"])
        return c if c else None

    return walk_right(s, b, min(len(s) - b, limit), K, base_at)


def md_both(x, y, seed_len):
    """MD:Z: over [a - eL, b + eR): the left mismatches from the left, the seed, the right mismatches; neighbouring match counts are one number"""
    out, prev = b"", 0
    for t, c in reversed(x["mis"][:x["nm"]]):
        u = x["ext"] - 1 - t
        out += b"%d" % (u - prev) + bytes([c])
        prev = u + 1
    run, at = x["ext"] - prev + seed_len, 0
    for t, c in y["mis"][:y["nm"]]:
        out += b"%d" % (run + t - at) + bytes([c])
        run, at = 0, t + 1
    return out + b"%d" % (run + y["ext"] - at)


ZERO = dict(ext=0, nm=0, score=0, steps=0, mis=[], why="none")


def read_records_both(o, fl, doc_starts, q, min_length, max_hits, secondary, K, resolve=None):
    """sam_extend_model.read_records with the right record of every line appended: (pick, j, l, dn, offs, x, y); y is ZERO (the same object) for a line
    that makes no item"""
    recs = XM.read_records(o, q, min_length, max_hits, secondary, K, resolve)
    if recs is None or recs == [None]:
        return recs
    srt = sorted(int(v) for v in doc_starts)
    out = []
    for p, j, l, dn, offs, x in recs:
        lo, hi, k, a, b, rev = p
        s = SAM.revcomp(q) if rev else bytes(q)
        y = ZERO
        if len(s) > b:
            start = l - offs
            nxt = [v for v in srt if v > start]
            doc_end = nxt[0] if nxt else fl.n
            seed_end = l + (b - a)
            if doc_end > seed_end:
                y = extend_right(fl, s, b, hi - (j - 1), b - a, doc_end - seed_end, max(K - x["nm"], 0))
        out.append((p, j, l, dn, offs, x, y))
    return out


def read_lines_both(o, fl, doc_starts, name, q, qual, min_length, max_hits, secondary, K, resolve=None):
    q, name = bytes(q), bytes(name)
    m = len(q)
    recs = read_records_both(o, fl, doc_starts, q, min_length, max_hits, secondary, K, resolve)
    if recs is None:
        return None
    if recs == [None]:
        return SAM.read_lines(o, name, q, qual, min_length, max_hits, secondary, resolve)
    out = []
    for (lo, hi, k, a, b, rev), j, l, dn, offs, x, y in recs:
        seq = SAM.revcomp(q) if rev else q
        ql = b"*" if qual is None else (bytes(qual)[::-1] if rev else bytes(qual))
        flag = (16 if rev else 0) | (256 if j > 1 else 0)
        e, er = x["ext"], y["ext"]
        out.append(b"\t".join([name, b"%d" % flag, dn, b"%d" % (offs + 1 - e), b"255", SAM.cigar(m, a - e, b + er), b"*", b"0", b"0", seq if j == 1 else b"*",
                               ql if j == 1 else b"*", b"NH:i:%d" % (hi - lo + 1), b"HI:i:%d" % j, b"NM:i:%d" % (x["nm"] + y["nm"]),
                               b"MD:Z:" + md_both(x, y, b - a), b"AS:i:%d" % (b - a + x["score"] + y["score"])]) + b"\n")
    return out


def lines_both(o, fl, doc_starts, names, seqs, quals, min_length=20, max_hits=16, secondary=False, K=4):
    cache = {}

    def resolve(l):
        if l not in cache:
            cache[l] = SAM.resolve_offset(o, l)
        return cache[l]

    out = []
    for i, (n, q) in enumerate(zip(names, seqs)):
        mine = read_lines_both(o, fl, doc_starts, n, q, None if quals is None else quals[i], min_length, max_hits, secondary, K, resolve)
        if mine is None:
            return None
        out += mine
    return out
