"""Test infrastructure: a plain-Python restatement of RowBowt::get_markers_lmems (reference include/rowbowt.hpp:341-404) on
the oracle's primitives (Oracle.LF, Oracle.markers_at, Oracle.find_range).  One record per end position e = m, m-1, ..., 1
of the query, in callback order: (lo, hi, q.first, q.second + 1, mbuf) -- the non-empty call of each end position.  The
reference's second call after a failed extension (:384-391 breaks out of the loop, then :402 runs with LF's empty range, the
same q and the cleared mbuf) carries nothing rb_markers prints (rb_markers.cpp:373 / :447 drop it)."""
import functools

ACGT = frozenset(b"ACGT")


def search_ftab(o, kmer):
    """search_ftab (rowbowt.hpp:746-758) on the table build_ftab(K) makes for this index (:726-744): its keys are the ACGT
    k-mers that occur, its values find_range's (oracle/rb_oracle.c ftab_hit).  A miss -- an absent k-mer, or any byte outside
    ACGT -- answers {full_range(), 0}, so the test at :371 never sees an empty range."""
    full = (0, o.n - 1)
    if not set(kmer) <= ACGT:
        return full
    lo, hi = o.find_range(bytes(kmer))
    return (lo, hi) if hi >= lo else full


def lmem_records(o, q, wsize, max_range, ftab_k=0):
    """-> [(lo, hi, qstart, qend_exclusive, [markers])], len(q) records (rowbowt.hpp:361-403)"""
    return [(a, b, c, d, list(mk)) for a, b, c, d, mk in _lmem_records(o, bytes(q), wsize, max_range, ftab_k)]


@functools.lru_cache(maxsize=None)
def _lmem_records(o, q, wsize, max_range, K):
    full = (0, o.n - 1)                               # full_range(), :115-118
    out = []
    m = len(q)
    for k in range(m):                                # :361
        e = m - k                                     # :363 (the reference's inner m)
        mbuf = []                                     # :362

        def update_mbuf(r):                           # :356-360 (markers_at appends)
            if r[1] - r[0] + 1 <= max_range:
                mbuf.extend(o.markers_at(r[0], r[1]))

        i, window_ei = 0, e                           # :365-366
        rng = prev = full                             # :367-368
        if K and e >= K:                              # :369 (a suffix shorter than K starts from the full range)
            rng = search_ftab(o, q[e - K:e])          # :370
            i += K                                    # :375 (a miss too: its full range is not empty)
            prev = rng                                # :376
        rec = None
        while i < e:                                  # :380
            prev = rng                                # :382
            rng = o.LF(rng[0], rng[1], q[e - i - 1])  # :383
            if rng[1] < rng[0]:                       # :384 the extension fails
                if i >= wsize:                        # :385 (m - (m - i) >= wsize)
                    update_mbuf(prev)
                rec = (prev[0], prev[1], e - i, e, tuple(mbuf))   # :389 fn(prev_range, (m-i, m-1), mbuf)
                break
            if window_ei - (e - i - 1) >= wsize:      # :393-396 (the ftab part never moved window_ei)
                update_mbuf(rng)
                window_ei = e - i - 1
            i += 1
        if rec is None:                               # :399-402 with i == m: the whole prefix q[0, e) occurs
            if i >= wsize:
                update_mbuf(rng)
            rec = (rng[0], rng[1], 0, e, tuple(mbuf))
        out.append(rec)
    return tuple(out)


class LmemAsGreedy:
    """Feeds rb_markers_model.expected_stdout lmem records: its `markers_greedy_seeding` hook returns them, so the model's
    rb_markers callback logic (worker / worker_heuristic, rb_markers.cpp:357-519) applies unchanged."""

    def __init__(self, o):
        self.o = o

    def markers_greedy_seeding(self, q, wsize, max_range, ftab_k=0):
        return lmem_records(self.o, q, wsize, max_range, ftab_k)
