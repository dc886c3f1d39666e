"""The doc_locs model of tests/test_gpu_locate_doc_hits.py (locations per document) against the oracle's resolve_offset, position by position, on the
tables that file runs the kernel with; and the identity that ties it to the other outputs: sum(doc_locs) + sum(nodoc) = the number of locations."""
import numpy as np
import pytest

import doc_hits_model as M
import orc
from rowbowt_amd import capi
from test_gpu_locate_doc_hits import TABLES, _starts, doc_locs_model, model


@pytest.mark.parametrize("kind", TABLES + [1025], ids=str)
def test_doc_locs_model_matches_the_oracle(synth, kind):
    S = synth
    starts = _starts(S, kind)
    names = [f"d{j}" for j in range(len(starts))]
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    o.set_docs(names, starts)
    size = (int(starts[-1]) + 1) & M.MAXU
    rng = np.random.default_rng(5)
    special = [0, 1, S.n - 1, S.n, size - 1, size, size + 1, M.MAXU, M.MAXU]
    for s in starts[:40] + starts[-40:]:
        special += [int(s) - 1, int(s), int(s) + 1]
    locs = np.array([v & M.MAXU for v in special] + rng.integers(0, S.n + 50, 2500).tolist(), dtype=np.uint64)
    rng.shuffle(locs)
    lens = rng.integers(0, 11, 400)
    lens[-1] = 0
    loc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert int(loc_off[-1]) <= len(locs)
    locs = locs[:int(loc_off[-1])]
    index = {n: j for j, n in enumerate(names)}
    want = np.zeros(len(starts), np.uint64)
    none = 0
    for l in locs.tolist():
        name, _ = o.resolve_offset(l)
        if name is None:
            none += 1
        else:
            want[index[name]] += np.uint64(1)
    o.close()
    got = doc_locs_model(locs, starts)
    assert got.dtype == np.uint64 and got.shape == want.shape and (got == want).all(), kind
    out = model(locs, loc_off, starts)
    assert (out["doc_locs"] == want).all()
    assert int(out["doc_locs"].sum()) + int(out["nodoc"].sum()) == len(locs) and int(out["nodoc"].sum()) == none
    # a document holds locations exactly when some read's set holds it
    assert ((out["doc_locs"] > 0) == (out["doc_reads"] > 0)).all()


def test_python_binding_surface_of_the_fused_calls():
    for m in ("locate_doc_hits", "doc_hits"):
        assert callable(getattr(capi.RowBowt, m)), m
    L = capi.lib()
    for f in ("rbg_locate_doc_hits_dev", "rbg_doc_hits_locs"):
        assert f in capi.EXPORTS and getattr(L, f).argtypes is not None, f
    assert capi.LOCATE_DOCS_MAX == 1024
    # no device: refused, never computed on the CPU
    assert L.rbg_locate_doc_hits_dev(None, None, None, None, 0, 0, None, None, None, None, None, None, None) == -3
