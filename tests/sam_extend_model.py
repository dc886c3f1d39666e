"""Test infrastructure: what rbg_extend_left_dev and rbg_align_sam_extend must produce (include/rbg.h; the rule: rowbowt_amd/csrc/rbg_sam.hpp), in Python
integers over Oracle.access (BWT[row]) and Oracle.LF (the one-row range stepped by a symbol), on top of sam_model.py.  Nothing here looks at the library.

    L = min(a, offs); score = best = 0; e = 0; nm = 0; mm = 0; r = r0
    for t in 0 .. L-1:
        c = BWT[r]                         one of A C G T, else stop
        x = s[a-1-t]
        if c == x: score += 1
        else: mm += 1; if mm > K: stop; score -= 4; remember (t, c)
        if score >= best: best = score; e = t + 1; nm = mm
        r = LF(r, c)
"""
import sam_model as SAM

MAX_MISMATCH = 8
ACGT = b"ACGT"
MATCH, MISMATCH = 1, -4


def walk_bases(s, a, L, K, base_at):
    """the rule over any source of reference bases: base_at(t) = the reference byte t + 1 positions left of the seed (None: there is none) -> a dict
    ext, nm, score, steps, mis = [(t, c), ...] every TAKEN mismatch in the order met (the first nm lie inside the extension), why = what ended the walk:
    'length' (L bases taken), 'budget' (the (K+1)-th mismatch), 'base' (a reference byte that is not A C G T)"""
    score = best = e = nm = mm = steps = 0
    mis, why = [], "length"
    for t in range(L):
        c = base_at(t)
        if c is None or c not in ACGT:
            why = "base"
            break
        x = s[a - 1 - t]
        if c == x:
            score += MATCH
        else:
            if mm + 1 > K:
                why = "budget"
                break
            mm += 1
            score += MISMATCH
            mis.append((t, c))
        if score >= best:
            best, e, nm = score, t + 1, mm
        steps += 1
    return dict(ext=e, nm=nm, score=best, steps=steps, mis=mis, why=why)


def extend(o, s, a, row, offs, K):
    """the rule over the index: BWT[r] by Oracle.access, r = LF(r, c) as the one-row range [r, r] stepped by c"""
    assert 0 <= K <= MAX_MISMATCH
    state = {"r": row, "t": -1}

    def base_at(t):
        assert t == state["t"] + 1                      # (walk_bases asks once per t, in order)
        if t > 0:
            lo, hi = o.LF(state["r"], state["r"], state["c"])
            assert lo == hi, (lo, hi)
            state["r"] = lo
        state["t"], state["c"] = t, o.access(state["r"])
        return state["c"]

    return walk_bases(bytes(s), a, min(a, offs), K, base_at)


def md(rec, seed_len):
    """MD:Z: over the read positions [a - e, b): match counts separated by the reference base of each mismatch inside the extension"""
    e, out, prev = rec["ext"], b"", 0
    for t, c in reversed(rec["mis"][:rec["nm"]]):
        u = e - 1 - t
        out += b"%d" % (u - prev) + bytes([c])
        prev = u + 1
    return out + b"%d" % (e - prev + seed_len)


def read_records(o, q, min_length, max_hits, secondary, K, resolve=None):
    """per line of one read: None (unmapped) or (pick, j, location, document name, offs, record); None for the whole read if a location lies before every
    document"""
    q = bytes(q)
    p = SAM.pick(o, q, min_length)
    if p is None:
        return [None]
    lo, hi, k, a, b, rev = p
    walk = max(max_hits, 1) if secondary else 1
    s = SAM.revcomp(q) if rev else q
    out = []
    for j, l in enumerate(o.locs_at(lo, hi, k, walk), 1):
        dn, offs = resolve(l) if resolve else SAM.resolve_offset(o, l)
        if dn is None:
            return None
        out.append((p, j, l, dn, offs, extend(o, s, a, hi - (j - 1), offs, K)))          # line j of [lo, hi] is row hi - (j - 1)
    return out


def read_lines(o, name, q, qual, min_length, max_hits, secondary, K, resolve=None):
    q, name = bytes(q), bytes(name)
    m = len(q)
    recs = read_records(o, q, min_length, max_hits, secondary, K, resolve)
    if recs is None:
        return None
    if recs == [None]:
        return SAM.read_lines(o, name, q, qual, min_length, max_hits, secondary, resolve)
    out = []
    for (lo, hi, k, a, b, rev), j, l, dn, offs, x in recs:
        seq = SAM.revcomp(q) if rev else q
        ql = b"*" if qual is None else (bytes(qual)[::-1] if rev else bytes(qual))
        flag = (16 if rev else 0) | (256 if j > 1 else 0)
        e = x["ext"]
        out.append(b"\t".join([name, b"%d" % flag, dn, b"%d" % (offs + 1 - e), b"255", SAM.cigar(m, a - e, b), b"*", b"0", b"0", seq if j == 1 else b"*",
                               ql if j == 1 else b"*", b"NH:i:%d" % (hi - lo + 1), b"HI:i:%d" % j, b"NM:i:%d" % x["nm"], b"MD:Z:" + md(x, b - a),
                               b"AS:i:%d" % (b - a + x["score"])]) + b"\n")
    return out


def lines(o, names, seqs, quals, min_length=20, max_hits=16, secondary=False, K=4):
    """every line of a batch in output order; None if a location lies before every document"""
    cache = {}

    def resolve(l):
        if l not in cache:
            cache[l] = SAM.resolve_offset(o, l)
        return cache[l]

    out = []
    for i, (n, q) in enumerate(zip(names, seqs)):
        mine = read_lines(o, n, q, None if quals is None else quals[i], min_length, max_hits, secondary, K, resolve)
        if mine is None:
            return None
        out += mine
    return out


def text(o, names, seqs, quals, min_length=20, max_hits=16, secondary=False, K=4):
    ls = lines(o, names, seqs, quals, min_length, max_hits, secondary, K)
    return None if ls is None else b"".join(ls)


def record_tuple(x):
    """a record as rbg_extend_t holds it: (ext, nm, score, steps, mis_t[8], mis_ref[8]) with unused entries zero"""
    t = [m[0] for m in x["mis"]] + [0] * (MAX_MISMATCH - len(x["mis"]))
    c = [m[1] for m in x["mis"]] + [0] * (MAX_MISMATCH - len(x["mis"]))
    return (x["ext"], x["nm"], x["score"], x["steps"], tuple(t), tuple(c))
