"""A numpy model of the document-hit calls (rbg_resolve_offsets_dev, rbg_doc_hits_dev; include/rbg.h) from (locs, loc_off, starts as given).

The rule is DocList::doc_and_offset_at (doclist.hpp:46-50) over doc_bounds_rank (:77-79): size = the LAST start given + 1 (:66, wrapping at 2^64);
for a position l, q = min(l + 1, size) with l + 1 wrapping; j = the number of starts < q; j == 0: no document; otherwise document j - 1 of the sorted
starts at offset l - sorted[j - 1].  tests/test_doc_hits_model.py checks it against the oracle's orc_resolve_offset."""
import numpy as np

DOC_NONE = 0xFFFFFFFF
MAXU = 2**64 - 1


def table(starts_given):
    """(sorted starts uint64, size)"""
    s = np.asarray(starts_given, dtype=np.uint64)
    return np.sort(s), (int(s[-1]) + 1) & MAXU


def resolve(locs, starts_given):
    """-> (doc uint32, DOC_NONE where a position has no document; offset uint64, the position itself there)"""
    srt, size = table(starts_given)
    l = np.asarray(locs, dtype=np.uint64)
    with np.errstate(over="ignore"):
        q = np.minimum(l + np.uint64(1), np.uint64(size))   # (l + 1 wraps to 0 at 2^64 - 1)
    j = np.searchsorted(srt, q, side="left")
    doc = np.where(j > 0, j - 1, DOC_NONE).astype(np.uint32)
    with np.errstate(over="ignore"):
        off = np.where(j > 0, l - srt[np.maximum(j, 1) - 1], l).astype(np.uint64)
    return doc, off


def widen32(locs32):
    """rbg_locate_fill_dev32's values as positions: 0xFFFFFFFF stands for the toehold that wrapped below zero"""
    v = np.asarray(locs32, dtype=np.uint32).astype(np.uint64)
    return np.where(v == 0xFFFFFFFF, np.uint64(MAXU), v)


def doc_hits(locs, loc_off, starts_given):
    """-> (sets[N, W] uint64, ndocs[N] uint32, nodoc[N] uint32, doc_reads[ndocs] uint64)"""
    nd = len(starts_given)
    W = (nd + 63) // 64
    loc_off = np.asarray(loc_off, dtype=np.uint64).astype(np.int64)
    N = len(loc_off) - 1
    doc, _ = resolve(locs, starts_given)
    read = np.repeat(np.arange(N, dtype=np.int64), np.diff(loc_off))
    doc = doc[:len(read)]
    none = doc == DOC_NONE
    nodoc = np.bincount(read[none], minlength=N).astype(np.uint32)
    member = np.zeros((N, W * 64), dtype=bool)
    member[read[~none], doc[~none].astype(np.int64)] = True
    ndocs = member.sum(axis=1).astype(np.uint32)
    doc_reads = member[:, :nd].sum(axis=0).astype(np.uint64)
    sets = np.ascontiguousarray(np.packbits(member, axis=1, bitorder="little")).view("<u8").astype(np.uint64).reshape(N, W)   # bit d % 64 of word d / 64
    return sets, ndocs, nodoc, doc_reads
