"""Test infrastructure: the bytes rbg_align_sam and rbg_sam_header must produce (include/rbg.h), built with Python integers on the oracle's
primitives: seeds_model.seeds_greedy / longest_seed on the read as given and on its reverse complement, Oracle.locs_at for the locations in
locate order, Oracle.resolve_offset for document and offset.  Nothing here looks at the library."""
import orc
import seeds_model as SM

MAXU = (1 << 64) - 1
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(q):
    """ACGTacgt -> TGCAtgca, every other byte itself (an N stays N), backwards"""
    return bytes(q).translate(_COMP)[::-1]


def cigar(m, a, b):
    return (b"%dS" % a if a else b"") + b"%dM" % (b - a) + (b"%dS" % (m - b) if m > b else b"")


def pick(o, q, min_length):
    """-> None (unmapped) or (lo, hi, k, a, b, rev): the longer of the two strands' longest greedy seeds, a tie to forward"""
    q = bytes(q)
    best = None
    for rev, s in ((0, q), (1, revcomp(q))):
        rec = SM.longest_seed(SM.seeds_greedy(o, s, min_length))
        if rec is not None and rec[1] >= rec[0] and (best is None or rec[3] - rec[2] > best[4] - best[3]):
            best = (rec[0], rec[1], rec[4], rec[2], rec[3], rev)
    return best


def resolve_offset(o, l):
    """the oracle's resolve_offset -> (name bytes, offset); (None, l): no document starts at or before l (an empty name is a name)"""
    off = orc.U64()
    name = o.L.orc_resolve_offset(o.h, l, off)
    return name, off.value


def read_lines(o, name, q, qual, min_length, max_hits, secondary, resolve=None):
    """the lines of one read (a list of bytes); None if a location lies before every document (the library answers RBG_EARG)"""
    q, name = bytes(q), bytes(name)
    m = len(q)
    p = pick(o, q, min_length)
    if p is None:
        return [b"\t".join([name, b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", q if m else b"*", qual if (qual is not None and m) else b"*"]) + b"\n"]
    lo, hi, k, a, b, rev = p
    walk = max(max_hits, 1) if secondary else 1
    locs = o.locs_at(lo, hi, k, walk)
    seq = revcomp(q) if rev else q
    ql = b"*" if qual is None else (bytes(qual)[::-1] if rev else bytes(qual))
    out = []
    for j, l in enumerate(locs, 1):
        dn, offs = resolve(l) if resolve else resolve_offset(o, l)
        if dn is None:
            return None
        flag = (16 if rev else 0) | (256 if j > 1 else 0)
        out.append(b"\t".join([name, b"%d" % flag, dn, b"%d" % (offs + 1), b"255", cigar(m, a, b), b"*", b"0", b"0", seq if j == 1 else b"*",
                               ql if j == 1 else b"*", b"NH:i:%d" % (hi - lo + 1), b"HI:i:%d" % j]) + b"\n")
    return out


def lines(o, names, seqs, quals, min_length=20, max_hits=16, secondary=False):
    """every line of a batch in output order; None as read_lines"""
    cache = {}

    def resolve(l):
        if l not in cache:
            cache[l] = resolve_offset(o, l)
        return cache[l]

    out = []
    for i, (n, q) in enumerate(zip(names, seqs)):
        mine = read_lines(o, n, q, None if quals is None else quals[i], min_length, max_hits, secondary, resolve)
        if mine is None:
            return None
        out += mine
    return out


def text(o, names, seqs, quals, min_length=20, max_hits=16, secondary=False):
    ls = lines(o, names, seqs, quals, min_length, max_hits, secondary)
    return None if ls is None else b"".join(ls)


def header(doc_names, doc_starts, n, pg=None):
    """@HD, one @SQ per document in sorted-start order -- name j of the list goes with the j-th smallest start, as the reference sorts the starts and
    not the names --, then pg as given"""
    srt = sorted(int(s) for s in doc_starts)
    out = b"@HD\tVN:1.6\tSO:unsorted\n"
    for j, s in enumerate(srt):
        end = srt[j + 1] if j + 1 < len(srt) else n
        name = doc_names[j].encode() if isinstance(doc_names[j], str) else doc_names[j]
        out += b"@SQ\tSN:%s\tLN:%d\n" % (name, max(end - s, 0))
    return out + (pg or b"")
