"""The numpy model of the document-hit calls (tests/doc_hits_model.py) against the oracle's resolve_offset, and the binding surface of the calls."""
import numpy as np
import pytest

import doc_hits_model as M
import orc
from rowbowt_amd import capi


def _positions(S, starts):
    n, size = S.n, (int(starts[-1]) + 1) & M.MAXU
    rng = np.random.default_rng(4)
    p = [0, 1, n - 2, n - 1, n, n + 1, size - 2, size - 1, size, size + 1, 2**32 - 1, 2**32, 2**63, M.MAXU - 1, M.MAXU]
    for s in starts:
        p += [int(s) - 1, int(s), int(s) + 1]
    p += rng.integers(0, n + 50, 3000).tolist()
    return np.array([v & M.MAXU for v in p], dtype=np.uint64)


def _tables(S):
    unit = S.L + S.pad
    asc = list(S.doc_starts)
    return {
        "synth": asc,
        "first start above 0": [s + 7 for s in asc],
        "last given smallest": asc[1:][::-1] + asc[:1],
        "last given in the middle": asc[:3] + asc[4:] + [asc[3]],
        "last given second largest": [asc[-1]] + asc[:-2] + [asc[-2]],
        "equal starts": [0, unit, unit, 3 * unit],
        "one document": [0],
    }


@pytest.mark.parametrize("which", ["synth", "first start above 0", "last given smallest", "last given in the middle", "last given second largest",
                                   "equal starts", "one document"])
def test_model_matches_the_oracle(synth, which):
    """resolve() against orc_resolve_offset, position by position: the offset, and the document through its NAME -- document d is entry d of the names AS
    GIVEN (doc_names_[rank - 1], doclist.hpp:49: the reference ranks over the sorted starts and indexes the names in file order; rbg_doc_table keeps
    that); a position without a document is one the oracle answers with no name"""
    S = synth
    starts = _tables(S)[which]
    names = [f"d{j}" for j in range(len(starts))]
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    o.set_docs(names, starts)
    srt = np.sort(np.array(starts, dtype=np.uint64))
    locs = _positions(S, starts)
    doc, off = M.resolve(locs, starts)
    none = 0
    for l, d, f in zip(locs.tolist(), doc.tolist(), off.tolist()):
        name, woff = o.resolve_offset(l)
        if name is None:
            assert d == M.DOC_NONE and f == l, (which, l)
            none += 1
        else:
            assert d != M.DOC_NONE and names[d] == name and f == woff == l - int(srt[d]), (which, l, d, name, f, woff)
    assert none >= (4 if which == "first start above 0" else 1)   # (2^64 - 1 always; 0, 1 and start - 1 below a first start of 7)
    o.close()


def test_doc_hits_model_on_a_hand_made_batch():
    """the four outputs on a batch small enough to write down"""
    starts = [100, 0, 50]            # as given: size = 51, sorted 0, 50, 100
    locs = np.array([0, 49, 50, 51, 99, 100, 200, M.MAXU,    # read 0: docs 0, 0, 1, 1 (q = 51 from 50 on: never beyond document 1), none for 2^64 - 1
                     7,                                     # read 2 (read 1 is empty)
                     M.MAXU, M.MAXU], dtype=np.uint64)        # read 3: no document twice
    loc_off = np.array([0, 8, 8, 9, 11], dtype=np.uint64)
    sets, ndocs, nodoc, doc_reads = M.doc_hits(locs, loc_off, starts)
    assert sets.shape == (4, 1) and sets[:, 0].tolist() == [0b11, 0, 0b01, 0]
    assert ndocs.tolist() == [2, 0, 1, 0] and nodoc.tolist() == [1, 0, 0, 2]
    assert doc_reads.tolist() == [2, 1, 0]
    doc, off = M.resolve(locs[:8], starts)
    assert doc.tolist() == [0, 0, 1, 1, 1, 1, 1, M.DOC_NONE] and off.tolist() == [0, 49, 0, 1, 49, 50, 150, M.MAXU]
    assert M.widen32(np.array([5, 0xFFFFFFFF, 0xFFFFFFFE], np.uint32)).tolist() == [5, M.MAXU, 0xFFFFFFFE]
    # more than 64 documents: the second word
    starts = [10 * j for j in range(130)]
    sets, ndocs, nodoc, doc_reads = M.doc_hits(np.array([5, 645, 1295, 1295], np.uint64), np.array([0, 4], np.uint64), starts)
    assert sets.shape == (1, 3) and sets[0].tolist() == [1, 1, 2] and ndocs.tolist() == [3] and int(doc_reads.sum()) == 3 and doc_reads[129] == 1


def test_python_binding_surface_of_the_document_calls():
    """the ctypes wrapper keeps the document-hit methods and binds their symbols (in the style of test_capi_host.test_python_binding_surface)"""
    for m in ("docs_prepare", "doc_hits_words", "resolve_offsets", "doc_hits", "doc_table"):
        assert callable(getattr(capi.RowBowt, m)), m
    L = capi.lib()
    for f in ("rbg_docs_prepare", "rbg_doc_hits_words", "rbg_resolve_offsets_dev", "rbg_resolve_offsets_dev32", "rbg_doc_hits_dev", "rbg_doc_hits_dev32",
              "rbg_doc_hits"):
        assert f in capi.EXPORTS and getattr(L, f).argtypes is not None, f
    assert (capi.DOCS_MAX, capi.DOC_NONE) == (1 << 16, 0xFFFFFFFF)
    # no device: refused, never computed on the CPU
    assert L.rbg_docs_prepare(None) == -4 and L.rbg_doc_hits_words(None) == 0
    assert L.rbg_doc_hits_dev(None, None, None, 0, None, None, None, None, None) == -3
    assert L.rbg_resolve_offsets_dev(None, None, 0, None, None, None) == -3
