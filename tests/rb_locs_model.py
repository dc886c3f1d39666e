"""Test infrastructure: a plain-Python restatement of what the reference's rb_locs does with each read (reference
src/rb_markers_tsa.cpp:76-88), on top of the oracle.  `o` holds the index (greedy_locate = find_locs_greedy_seeding); `ot` is a second
Oracle whose marker array holds the runs of the TEXT-position table (<prefix>.midx): its interval query markers_at(lo, hi) -- every run
with end >= lo and start <= hi, nothing when hi < lo -- does not depend on its BWT.  The expected stdout of the rb_locs-compatible CLI and
the expected output of rbg_markers_at_locs / rbg_find_loc_markers_greedy_seeding are computed with it."""
import golden_values as G
from rb_markers_model import get_seq

M64 = 2**64 - 1


def markers_at_loc(ot, l, m):
    """midx.at_range(l, l + m - 1) in wrapping 64-bit arithmetic (:82): empty when the end lies below the start (m == 0, or a location that
    wrapped below zero whose end wraps back); a start at or beyond n meets no run; an end beyond the text meets the runs up to n - 1"""
    return ot.markers_at(l, (l + m - 1) & M64)


def loc_markers(o, ot, q, min_length=10, max_hits=M64):
    """(locations, markers) of one read: the markers location after location, run order within a location (:80-86)"""
    locs = o.greedy_locate(q, min_length, max_hits)[0]
    mk = []
    for l in locs:
        mk += markers_at_loc(ot, l, len(q))
    return locs, mk


def expected_stdout(o, ot, records, wsize=10, max_hits=M64):
    """records = [(name bytes, seq bytes)] in file order -> the text rb_locs prints: the read as it stands in the file (no nt table, no
    reverse complement), its name, then " seq/pos/allele" per marker"""
    out = []
    for name, seq in records:
        _locs, mk = loc_markers(o, ot, seq, wsize, max_hits)
        out.append(name.decode() + "".join(f" {get_seq(m)}/{G.get_pos(m)}/{G.get_allele(m)}" for m in mk) + "\n")
    return "".join(out)
