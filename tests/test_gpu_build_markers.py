"""rbg_build_from_text_markers / rbg_convert_text_markers (capi/build_text.ipp) on the GPU: the index RowBowt.from_text(text, markers=(pos, first, val, w))
builds answers every marker query exactly as RowBowt.from_runs of the same text's run arrays with set_markers(the model's arrays) does -- on the text the
reference's fixture was built over (there the marker goldens of tests/golden/reference_rb_tests.json hold as well) and on the three documents
of tests/marker_build_cases.py with windows of 19.  The cache file is compared byte for byte, and markers=None is the build of before."""
import functools

import numpy as np
import pytest
import torch

import golden_values as G
import marker_build_cases as MC
import marker_build_model as MB
import rowbowt_amd as ra
import sa_scale_cases as SC
from rowbowt_amd import capi

pytestmark = pytest.mark.gpu
MAXU = G.MAXU
ARRAYS = (capi.ARR_RUN_HEADS, capi.ARR_RUN_START, capi.ARR_SAMPLES_LAST, capi.ARR_PRED_POS, capi.ARR_PHI_BASE)


@functools.lru_cache(maxsize=None)
def case(name):
    """text, records, w, the run arrays and the model's marker arrays: made once"""
    if name == "fixture":
        F = MB.fixture_layout(10)
        text, rec, w = F["text"], (F["pos"], F["first"], F["val"]), 10
    else:
        text, rec, w = MC.edge_text(), MC.edge_records(19), 19
    sa = capi.suffix_array(torch.from_numpy(text).cuda()).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    return dict(text=text, rec=rec, w=w, sa=sa, runs=SC.runs_from_sa(text, sa), mk=MB.marker_runs(sa, *rec))


def pair(name):
    c = case(name)
    rb = ra.RowBowt.from_text(c["text"], device=0, markers=c["rec"] + (c["w"],))
    want = ra.RowBowt.from_runs(*c["runs"], device=0)
    want.set_markers(*c["mk"])
    return c, rb, want


def windows(c, length, step):
    """reads cut from the text around every site, and a few that match nowhere"""
    t = bytes(c["text"])
    reads = []
    for p in c["rec"][0].tolist()[::step]:
        for a in (p - length + 1, p - length // 2, p):
            r = t[max(a, 0):max(a, 0) + length]
            if r and b"\x01" not in r and b"#" not in r:
                reads.append(r)
    return reads + [b"ACGT" * 6, b"T" * 30]


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.asarray(x).shape == np.asarray(y).shape and (np.asarray(x) == np.asarray(y)).all()


@pytest.mark.parametrize("name", ["fixture", "edges"])
def test_marker_queries_are_those_of_the_model_arrays(name, simple_reads, error_reads):
    c, rb, want = pair(name)
    try:
        assert rb.info().has_markers == 1 and rb.info().n == len(c["text"])
        for which in ARRAYS:
            assert (rb.host_array(which) == want.host_array(which)).all(), which
        reads = windows(c, 20, 1 if name == "edges" else 3) + (simple_reads + error_reads if name == "fixture" else [])
        seqs, off = ra.pack_reads(reads)
        got = rb.find_range_w_markers(seqs, off, c["w"], MAXU)
        same(got, want.find_range_w_markers(seqs, off, c["w"], MAXU))
        assert int(got[2][-1]) > 0
        # every range of widths 1 to 3 around each run edge
        s, e = c["mk"][0].astype(np.int64), c["mk"][1].astype(np.int64)
        n = len(c["text"])
        lo = np.unique(np.concatenate([x + d for x in (s, e) for d in range(-3, 2)]))
        lo = lo[(lo >= 0) & (lo < n)]
        for width in (1, 2, 3):
            hi = np.minimum(lo + width - 1, n - 1)
            g = rb.markers_at(lo, hi)
            same(g, want.markers_at(lo, hi))
            assert int(g[0][-1]) > 0
        for wsize, ftab_k in ((c["w"], 0), (4, 0)):
            g = rb.get_markers_greedy_seeding(seqs, off, wsize, MAXU, ftab_k)
            same(g, want.get_markers_greedy_seeding(seqs, off, wsize, MAXU, ftab_k))
            assert len(g[2]) > 0
    finally:
        rb.close(), want.close()


def test_the_marker_goldens_hold_on_the_fixture_layout(simple_reads):
    c = case("fixture")
    rb = ra.RowBowt.from_text(c["text"], device=0, markers=c["rec"] + (c["w"],))
    try:
        seqs, off = ra.pack_reads(simple_reads)
        lo, hi, mk_off, mk = rb.find_range_w_markers(seqs, off, 10, MAXU)      # rb_tests.cpp:126
        assert list(zip(lo.tolist(), hi.tolist())) == G.SIMPLE_RANGES
        for i, want in enumerate(G.SIMPLE_FIRST_MARKER):                     # rb_tests.cpp:131-140
            got = mk[int(mk_off[i]):int(mk_off[i + 1])].tolist()
            if want is None:
                assert got == []
            else:
                assert (G.get_pos(got[0]), G.get_allele(got[0])) == want
    finally:
        rb.close()


@pytest.mark.parametrize("name", ["fixture", "edges"])
def test_cache_file_is_the_one_from_the_model_arrays(name, tmp_path):
    c = case(name)
    docs_text = "ref 0\nhap1 10010\nhap2 20020\n" if name == "fixture" else "a 0\nb 151\nc 249\n"
    a, b = tmp_path / "text.rbgpu", tmp_path / "runs.rbgpu"
    capi.convert_text_markers(c["text"], c["rec"] + (c["w"],), a, docs_text=docs_text)
    capi.convert_runs(*c["runs"], out_path=b, markers=c["mk"], docs_text=docs_text)
    assert a.read_bytes() == b.read_bytes()


def test_without_markers_the_build_is_the_one_of_before(tmp_path):
    c = case("edges")
    z = np.zeros(0, np.uint64)
    plain = ra.RowBowt.from_text(c["text"], device=0)
    none = ra.RowBowt.from_text(c["text"], device=0, markers=None)
    empty = ra.RowBowt.from_text(c["text"], device=0, markers=(z, z, z, 0))      # S == 0: w is not looked at
    want = ra.RowBowt.from_runs(*c["runs"], device=0)
    try:
        for rb in (plain, none, empty):
            assert rb.info().has_markers == 0
            for which in ARRAYS:
                assert (rb.host_array(which) == want.host_array(which)).all(), which
    finally:
        for rb in (plain, none, empty, want):
            rb.close()
    a, b = tmp_path / "a.rbgpu", tmp_path / "b.rbgpu"
    capi.convert_text(c["text"], a)
    capi.convert_text_markers(c["text"], (z, z, z, 0), b)
    assert a.read_bytes() == b.read_bytes()


def test_records_that_break_the_rule_are_refused():
    c = case("edges")
    pos, first, val = (a.copy() for a in c["rec"])
    L = ra.lib()
    h = capi.VP()

    def build(p, f, v, S, w):
        return L.rbg_build_from_text_markers(capi._p(c["text"]), len(c["text"]), capi._p(p), capi._p(f), capi._p(v), S, w, 1, 0, capi.C.byref(h))

    swapped = pos.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    assert build(swapped, first, val, len(pos), 19) == -4 and not h.value
    assert build(pos, first, val, len(pos), 0) == -4 and build(pos, first, val, len(pos), 65) == -4 and not h.value
    assert build(pos, first, val, len(pos), 18) == -4 and not h.value                       # a window of 19 under w = 18
    assert build(None, first, val, len(pos), 19) == -4 and not h.value
    assert L.rbg_build_from_text_markers(capi._p(c["text"]), len(c["text"]), capi._p(pos), capi._p(first), capi._p(val), len(pos), 19, 1, capi.DEVICE_NONE,
                                         capi.C.byref(h)) == -3
    assert build(pos, first, val, len(pos), 19) == 0 and h.value
    L.rbg_free(h)
