"""Document hits from the phi walk itself (include/rbg.h rbg_locate_doc_hits_dev, rbg_doc_hits_locs; rbg_locate_docs.hpp): one kernel walks each read's
chain and reduces its positions into the document set, nothing stored per location.  Every case runs on six index forms -- the slot layout and the
run-indexed one with phi slots and with the phi list, each at 4- and 8-byte positions -- against the oracle's find_range_w_toehold_batch + locs_at_batch
reduced by tests/doc_hits_model.py (plus doc_locs_model below: locations per document), and against the two-step device pipeline (plan + fill +
rbg_doc_hits_dev) in the same test, so that a difference names its side.  Every read of every batch is compared; every comparison is exact."""
import os
import re

import numpy as np
import pytest

import doc_hits_model as M
import orc
import rowbowt_amd as ra
from rowbowt_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXU = M.MAXU
ENOTLOADED, EARG = -6, -4
OUTPUTS = ("sets", "ndocs", "nodoc", "doc_reads", "doc_locs")
FORMS = [(capi.LAYOUT_SLOTS, 0, 4), (capi.LAYOUT_SLOTS, 0, 8), (capi.LAYOUT_RUNS, 2, 4), (capi.LAYOUT_RUNS, 2, 8), (capi.LAYOUT_RUNS, 1, 4), (capi.LAYOUT_RUNS, 1, 8)]
FORM_IDS = ["slots-pos4", "slots-pos8", "runs-phislots-pos4", "runs-phislots-pos8", "runs-philist-pos4", "runs-philist-pos8"]


def doc_locs_model(locs, starts_given):
    """locations per document: bincount of the model's documents (tests/test_locate_doc_hits_model.py holds it to the oracle's resolve_offset)"""
    doc, _ = M.resolve(locs, starts_given)
    return np.bincount(doc[doc != M.DOC_NONE].astype(np.int64), minlength=len(starts_given)).astype(np.uint64)


def model(locs, loc_off, starts):
    sets, ndocs, nodoc, doc_reads = M.doc_hits(locs, loc_off, starts)
    return {"sets": sets, "ndocs": ndocs, "nodoc": nodoc, "doc_reads": doc_reads, "doc_locs": doc_locs_model(locs[:int(loc_off[-1])], starts)}


def _const(name, header):
    src = open(os.path.join(ROOT, "rowbowt_amd", "csrc", header)).read()
    m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, src)
    assert m, f"constexpr uint32_t {name} = <decimal>; not found in {header}: this file's boundary cases follow that constant"
    return int(m.group(1))


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}[a.dtype]
    return torch.from_numpy(a.view(view)).cuda()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _order(rb, d_k, N):
    import torch
    L = ra.lib()
    ws_bytes = L.rbg_locate_order_ws_bytes(N)
    d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    assert L.rbg_locate_order_dev(rb.h, d_k.data_ptr(), N, d_ws.data_ptr(), ws_bytes, _stream()) == 0
    return d_ws


def _fused(rb, d_lo, d_hi, d_k, N, nd, max_hits=MAXU, ordered=False, only=OUTPUTS, held=None):
    """one rbg_locate_doc_hits_dev call -> the outputs named in `only` (the others are passed as NULL and come back as None; their buffers must be
    untouched) and the rbg_counters delta of the call.  held: {doc_reads / doc_locs: what the array holds before the call}"""
    import torch
    L = ra.lib()
    W = (nd + 63) // 64
    out = {"sets": torch.full((N * W + 1,), -1, dtype=torch.int64, device="cuda"), "ndocs": torch.full((N + 1,), -1, dtype=torch.int32, device="cuda"),
           "nodoc": torch.full((N + 1,), -1, dtype=torch.int32, device="cuda")}
    for k in ("doc_reads", "doc_locs"):
        out[k] = _t(np.concatenate([np.zeros(nd, np.uint64) if not held or k not in held else np.asarray(held[k], dtype=np.uint64), [np.uint64(MAXU)]]))
    ptr = {k: (v.data_ptr() if k in only else None) for k, v in out.items()}
    d_ws = _order(rb, d_k, N) if ordered and N else None
    before = rb.counters().copy()
    rc = L.rbg_locate_doc_hits_dev(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), d_k.data_ptr(), N, max_hits, d_ws.data_ptr() if d_ws is not None else None,
                                   ptr["sets"], ptr["ndocs"], ptr["nodoc"], ptr["doc_reads"], ptr["doc_locs"], _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    delta = rb.counters() - before
    size = {"sets": N * W, "ndocs": N, "nodoc": N, "doc_reads": nd, "doc_locs": nd}
    view = {"sets": np.uint64, "ndocs": np.uint32, "nodoc": np.uint32, "doc_reads": np.uint64, "doc_locs": np.uint64}
    res = {}
    for k, v in out.items():
        h = v.cpu().numpy().view(view[k])
        assert h[size[k]] == (MAXU if view[k] == np.uint64 else 0xFFFFFFFF), ("written behind its end", k)
        if k in only:
            res[k] = h[:size[k]].reshape(N, W) if k == "sets" else h[:size[k]]
        else:
            fill = (held or {}).get(k, 0) if k in ("doc_reads", "doc_locs") else (MAXU if k == "sets" else 0xFFFFFFFF)
            assert (h[:size[k]] == fill).all(), ("a NULL output's buffer was written", k)
            res[k] = None
    return res, delta


def _two_step(rb, d_lo, d_hi, d_k, N, nd, max_hits=MAXU, ordered=True):
    """rbg_locate_plan_dev + [order] + rbg_locate_fill_dev + rbg_doc_hits_dev on the same arrays -> (outputs -- doc_locs by the model from the stored
    locations --, loc_off, locs, the rbg_counters delta)"""
    import torch
    L = ra.lib()
    W = (nd + 63) // 64
    st = _stream()
    d_loc_off = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    tmp_bytes = L.rbg_locate_plan_tmp_bytes(N)
    d_tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device="cuda")
    before = rb.counters().copy()
    assert L.rbg_locate_plan_dev(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), N, max_hits, d_loc_off.data_ptr(), d_tmp.data_ptr(), tmp_bytes, st) == 0
    total = int(d_loc_off[-1].item())
    d_locs = torch.full((total + 1,), -1, dtype=torch.int64, device="cuda")
    d_ws = _order(rb, d_k, N) if ordered and N else None
    assert L.rbg_locate_fill_dev(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), d_k.data_ptr(), N, max_hits, d_loc_off.data_ptr(), d_locs.data_ptr(),
                                 d_ws.data_ptr() if d_ws is not None else None, st) == 0
    d_sets = torch.zeros(N * W + 1, dtype=torch.int64, device="cuda")
    d_nd, d_no = (torch.zeros(N + 1, dtype=torch.int32, device="cuda") for _ in range(2))
    d_dr = torch.zeros(nd, dtype=torch.int64, device="cuda")
    assert L.rbg_doc_hits_dev(rb.h, d_locs.data_ptr(), d_loc_off.data_ptr(), N, d_sets.data_ptr(), d_nd.data_ptr(), d_no.data_ptr(), d_dr.data_ptr(), st) == 0
    torch.cuda.synchronize()
    delta = rb.counters() - before
    loc_off, locs = d_loc_off.cpu().numpy().view(np.uint64), d_locs[:total].cpu().numpy().view(np.uint64)
    starts = rb.doc_table(names=False)[1]   # (sorted: the model's documents index the sorted starts either way; size needs the last GIVEN start)
    res = {"sets": d_sets[:N * W].cpu().numpy().view(np.uint64).reshape(N, W), "ndocs": d_nd[:N].cpu().numpy().view(np.uint32),
           "nodoc": d_no[:N].cpu().numpy().view(np.uint32), "doc_reads": d_dr.cpu().numpy().view(np.uint64)}
    return res, loc_off, locs, delta, starts


def _same(got, want, what):
    for k in OUTPUTS:
        if got.get(k) is not None and want.get(k) is not None:
            g, w = got[k], want[k]
            assert g.shape == w.shape, (what, k, g.shape, w.shape)
            assert (g == w).all(), (what, k, np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))[:5])


def _check(rb, d, N, starts, want, what, max_hits=MAXU, orders=(False, True)):
    """the fused call, unordered and ordered, against `want` (the model over the oracle's locations) and against the two-step pipeline, counters included"""
    nd = len(starts)
    two, loc_off, locs, two_delta, _ = _two_step(rb, *d, N, nd, max_hits)
    two["doc_locs"] = doc_locs_model(locs, starts)
    _same(two, want, (what, "two-step against the model"))
    for ordered in orders:
        got, delta = _fused(rb, *d, N, nd, max_hits, ordered)
        _same(got, want, (what, "fused against the model", "ordered" if ordered else "unordered"))
        _same(got, two, (what, "fused against the two-step pipeline", "ordered" if ordered else "unordered"))
        assert delta.tolist() == two_delta.tolist() == [0, 0, 0, int(loc_off[-1])], (what, ordered, delta, two_delta)
        assert int(got["doc_locs"].sum()) + int(got["nodoc"].sum()) == int(delta[3]), what


def _search(rb, seqs, off):
    import torch
    L = ra.lib()
    N = len(off) - 1
    d_seqs = torch.from_numpy(np.concatenate([seqs, np.zeros((-len(seqs)) % 16 + 16, np.uint8)])).cuda()
    d_off = _t(off)
    d = tuple(torch.zeros(max(N, 1), dtype=torch.int64, device="cuda") for _ in range(3))
    assert L.rbg_find_range_w_toehold_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    return d


@pytest.fixture(scope="module")
def oracle(synth):
    o = orc.Oracle.from_runs(synth.heads, synth.lens, synth.ssa, synth.esa)
    yield o
    o.close()


@pytest.fixture(scope="module", params=FORMS, ids=FORM_IDS)
def handle(request, synth):
    S = synth
    layout, phi, pos_bytes = request.param
    with capi.default_option(capi.OPT_RANK_LAYOUT, layout), capi.default_option(capi.OPT_RUN_PHI, phi), capi.default_option(capi.OPT_POS_BYTES, pos_bytes):
        rb = ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0)
    assert rb.info().pos_bytes == pos_bytes
    yield rb
    rb.close()


@pytest.fixture(scope="module")
def searched(synth, oracle):
    """the reads of test_gpu_doc_hits.pipeline_case plus an empty one, one with an unknown symbol and a prefix of the text; their ranges, toeholds and,
    per max_hits, locations from the oracle"""
    S, o = synth, oracle
    reads = [r for r in S.sample_reads(2500, 40, seed=31, sub_rate=0.1, ragged=True) if len(r) >= 2] + [bytes(S.text[:30]), b"AC", b"ACGTNACGT", b"TTTTTTTTTTTTTTTTTTTTTTTTT"]
    reads += [b"", b"ACGTN", bytes(S.text[:30])]
    seqs, off = ra.pack_reads(reads)
    wlo, whi, wk = o.find_range_w_toehold_batch(seqs, off, nthreads=4)
    occ = np.where(whi >= wlo, whi - wlo + np.uint64(1), np.uint64(0))
    assert int(occ.max()) > 1000 and int((occ == 0).sum()) > 10   # counts from thousands to none
    locs = {mh: o.locs_at_batch(wlo, whi, wk, mh, nthreads=4) for mh in (MAXU, 2, 1, 0)}
    return reads, seqs, off, wlo, whi, wk, locs


def _ranges_on(rb, searched):
    reads, seqs, off, wlo, whi, wk, _ = searched
    d = _search(rb, seqs, off)
    for g, w in zip(d, (wlo, whi, wk)):
        assert (g.cpu().numpy().view(np.uint64) == w).all()
    return d, len(reads)


def test_searched_reads(synth, handle, searched):
    """reads with none to thousands of locations, max_hits unlimited, 2, 1 and 0, with d_order NULL and with the order workspace: all five outputs and
    the rbg_counters delta equal the model's and the two-step path's"""
    S, rb = synth, handle
    rb.set_docs(S.doc_names, S.doc_starts)
    rb.docs_prepare()
    d, N = _ranges_on(rb, searched)
    for mh in (MAXU, 2, 1, 0):
        woff, wlocs = searched[6][mh]
        _check(rb, d, N, S.doc_starts, model(wlocs, woff, S.doc_starts), ("max_hits", mh), mh)


def test_wrapped_toeholds(synth, handle, oracle, monkeypatch):
    """a toehold that wrapped below zero (2^64 - 1), planted on two reads of several locations as test_gpu_doc_hits.test_32_bit_locations does: the
    location has no document, and the walk goes on with phi's arithmetic outside its domain.  Ordered, the kernel reads d_k[i] itself behind the 32-bit
    key 0xFFFFFFFF (4-byte positions, absolute order) and behind the all-ones locus key (RBG_LOCATE_ORDER=locus)"""
    import torch
    S, rb, o = synth, handle, oracle
    reads = S.sample_reads(1500, 40, seed=21, sub_rate=0.1) + [bytes(S.text[:40]), bytes(S.text[:25]), bytes(S.text[1:30]), b"", b"ACGTN"]
    seqs, off = ra.pack_reads(reads)
    N = len(reads)
    wlo, whi, wk = o.find_range_w_toehold_batch(seqs, off, nthreads=4)
    wk = wk.copy()
    multi = np.flatnonzero(whi - wlo + 1 >= 3)[:2]
    assert len(multi) == 2
    wk[multi] = np.uint64(MAXU)
    woff, wlocs = o.locs_at_batch(wlo, whi, wk, nthreads=4)
    assert (wlocs == np.uint64(MAXU)).any(), "no wrapped toehold among the locations: the case this test is about is missing"
    want = model(wlocs, woff, S.doc_starts)
    assert int(want["nodoc"][multi].min()) >= 1   # the wrapped toeholds have no document
    for order in ("abs", "locus"):
        monkeypatch.setenv("RBG_LOCATE_ORDER", order)
        rb.set_docs(S.doc_names, S.doc_starts)
        rb.docs_prepare()
        d = _search(rb, seqs, off)
        d[2].copy_(torch.from_numpy(wk.view(np.int64)))
        _check(rb, d, N, S.doc_starts, want, ("wrapped", order))
    monkeypatch.delenv("RBG_LOCATE_ORDER")
    rb.set_docs(S.doc_names, S.doc_starts)


def _starts(S, kind):
    """the starts AS GIVEN of one table of the list (as test_gpu_doc_hits._starts)"""
    rng = np.random.default_rng(17)
    if isinstance(kind, int):
        if kind == 1:
            return [0]
        return [0] + np.sort(rng.choice(np.arange(1, S.n - 1), size=kind - 1, replace=False)).tolist()
    if kind == "first start above 0":
        return [s + 123 for s in S.doc_starts]
    assert kind == "out of order"
    s = list(S.doc_starts)
    return [s[5], s[0], s[7], s[2], s[1], s[6], s[4], s[3]]   # the last given start lies in the middle: size = s[3] + 1


TABLES = [1, 2, 64, 65, 128, 129, 1024, "first start above 0", "out of order"]


def test_tables(synth, handle, searched):
    """hand-made starts over the same text: real chains, arbitrary documents, from one document to the most the kernel stages (from 128 on the chains are
    ordered by locus); one document more is refused by the device call and answered by the host call through the two-step path"""
    S, rb = synth, handle
    L = ra.lib()
    lds = _const("kLocDocLdsDocs", "rbg_dev.h")
    assert lds == 1024 == capi.LOCATE_DOCS_MAX and 2 * (lds + 1) < S.n
    d, N = _ranges_on(rb, searched)
    reads, seqs, off, wlo, whi, wk, locs = searched
    woff, wlocs = locs[MAXU]
    for kind in TABLES:
        starts = _starts(S, kind)
        rb.set_docs([f"d{j}" for j in range(len(starts))], starts)
        rb.docs_prepare()
        want = model(wlocs, woff, starts)
        if kind != 1:
            assert int(want["ndocs"].max()) >= 2
        _check(rb, d, N, starts, want, ("table", kind))
    starts = _starts(S, lds + 1)
    rb.set_docs([f"d{j}" for j in range(lds + 1)], starts)
    rb.docs_prepare()
    assert L.rbg_locate_doc_hits_dev(rb.h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), N, MAXU, None, None, None, None, None, None, _stream()) == EARG
    want = model(wlocs, woff, starts)
    lo, hi, sets, ndocs, nodoc, doc_reads, doc_locs = rb.doc_hits(seqs, off, MAXU, doc_locs=True)
    assert (lo == wlo).all() and (hi == whi).all()
    _same({"sets": sets, "ndocs": ndocs, "nodoc": nodoc, "doc_reads": doc_reads, "doc_locs": doc_locs}, want, "host call above the kernel's table limit")
    rb.set_docs(S.doc_names, S.doc_starts)


def test_batch_edges(synth, handle, searched):
    """N = 0, 1 and around a wave and a workgroup; every output NULL still walks (the counters move); every output alone, since the instantiation with
    doc_locs and the plain one are different kernels"""
    S, rb = synth, handle
    L = ra.lib()
    rb.set_docs(S.doc_names, S.doc_starts)
    rb.docs_prepare()
    reads, seqs, off, wlo, whi, wk, _ = searched
    first = int(np.flatnonzero(whi >= wlo)[0])   # (so that the batch of one read has a location)
    for N in (0, 1, 63, 64, 65, 257):
        sub = reads[first:first + N]
        s2, o2 = ra.pack_reads(sub) if N else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
        d = _search(rb, s2, o2)
        woff, wlocs = (np.zeros(1, np.uint64), np.zeros(0, np.uint64)) if N == 0 else _oracle_locs(searched, first, N)
        want = model(wlocs, woff, S.doc_starts)
        _check(rb, d, N, S.doc_starts, want, ("N", N))
        got, delta = _fused(rb, *d, N, S.H, only=())
        assert delta.tolist() == [0, 0, 0, len(wlocs)], N
        for one in OUTPUTS:
            for ordered in (False, True):
                got, delta = _fused(rb, *d, N, S.H, ordered=ordered, only=(one,))
                _same(got, want, ("N", N, "only", one, ordered))
                assert delta.tolist() == [0, 0, 0, len(wlocs)]
    assert L.rbg_locate_doc_hits_dev(rb.h, None, d[1].data_ptr(), d[2].data_ptr(), 5, MAXU, None, None, None, None, None, None, _stream()) == EARG
    assert L.rbg_locate_doc_hits_dev(rb.h, d[0].data_ptr(), None, d[2].data_ptr(), 5, MAXU, None, None, None, None, None, None, _stream()) == EARG
    assert L.rbg_locate_doc_hits_dev(rb.h, d[0].data_ptr(), d[1].data_ptr(), None, 5, MAXU, None, None, None, None, None, None, _stream()) == EARG
    assert L.rbg_locate_doc_hits_dev(rb.h, None, None, None, 0, MAXU, None, None, None, None, None, None, _stream()) == 0


def _oracle_locs(searched, first, N):
    """the oracle's locations of reads [first, first + N) cut out of the whole batch's"""
    woff, wlocs = searched[6][MAXU]
    a, b = int(woff[first]), int(woff[first + N])
    return (woff[first:first + N + 1] - woff[first]).astype(np.uint64), wlocs[a:b]


def test_accumulation(synth, handle, searched):
    """two calls into d_doc_reads and d_doc_locs that were not zeroed: what they held plus both batches"""
    S, rb = synth, handle
    rb.set_docs(S.doc_names, S.doc_starts)
    rb.docs_prepare()
    d, N = _ranges_on(rb, searched)
    rng = np.random.default_rng(10)
    held = {"doc_reads": rng.integers(1, 1000, S.H).astype(np.uint64), "doc_locs": rng.integers(1, 1000, S.H).astype(np.uint64)}
    total = {k: v.copy() for k, v in held.items()}
    for mh in (MAXU, 2):
        woff, wlocs = searched[6][mh]
        want = model(wlocs, woff, S.doc_starts)
        got, _ = _fused(rb, *d, N, S.H, mh, ordered=True, held=total)
        total = {k: total[k] + want[k] for k in total}
        assert (got["doc_reads"] == total["doc_reads"]).all() and (got["doc_locs"] == total["doc_locs"]).all()
    assert all((total[k] > held[k]).all() for k in held)


@pytest.fixture(scope="module")
def stride_case(synth):
    """more reads than the largest grid has lanes: hand-made (lo, hi, k) from the text's suffix array (tests/text_ref.py), no search -- ranges of 0 to 2
    rows at random rows, k = SA[hi], expected positions SA[hi], SA[hi - 1], ..."""
    from text_ref import TextRef
    S = synth
    cap, block = _const("kLocDocMaxBlocks", "rbg_locate_docs.hpp"), _const("kLocDocBlock", "rbg_locate_docs.hpp")
    N = cap * block + 1000
    assert N > cap * block
    ref = TextRef(S.text, S.fm.sa)
    rng = np.random.default_rng(12)
    width = rng.integers(0, 3, N)
    row = rng.integers(0, S.n - 2, N)
    lo = np.where(width > 0, row, 1).astype(np.uint64)
    hi = np.where(width > 0, row + width - 1, 0).astype(np.uint64)
    k = ref.toehold(lo, hi)
    loc_off, locs = ref.locs(lo, hi)
    assert int(loc_off[-1]) == int(width.sum())
    return N, lo, hi, k, model(locs, loc_off, S.doc_starts), int(loc_off[-1])


def test_grid_stride(synth, handle, stride_case):
    """the kernel's loop goes round: the grid cap times the workgroup plus 1000 reads"""
    S, rb = synth, handle
    rb.set_docs(S.doc_names, S.doc_starts)
    rb.docs_prepare()
    N, lo, hi, k, want, total = stride_case
    d = (_t(lo), _t(hi), _t(k))
    for ordered in (False, True):
        got, delta = _fused(rb, *d, N, S.H, ordered=ordered)
        _same(got, want, ("grid stride", ordered))
        assert delta.tolist() == [0, 0, 0, total]
    got, _ = _fused(rb, *d, N, S.H, ordered=True, only=("sets", "ndocs", "nodoc", "doc_reads"))   # (the instantiation without doc_locs)
    _same(got, want, "grid stride, no doc_locs")


def test_replica(synth, handle, searched):
    """a replica answers RBG_ENOTLOADED until it has prepared its own copy of the table, then gives the primary's outputs; rbg_set_docs on the primary
    makes it stale again"""
    S, rb = synth, handle
    L = ra.lib()
    rb.set_docs(S.doc_names, S.doc_starts)
    woff, wlocs = searched[6][MAXU]
    want = model(wlocs, woff, S.doc_starts)
    rep = rb.replicate(0)
    try:
        d, N = _ranges_on(rep, searched)

        def bare():
            return L.rbg_locate_doc_hits_dev(rep.h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), N, MAXU, None, None, None, None, None, None, _stream())
        assert bare() == ENOTLOADED
        rep.docs_prepare()
        for ordered in (False, True):
            got, _ = _fused(rep, *d, N, S.H, ordered=ordered)
            _same(got, want, ("replica", ordered))
        other = [s + 5 for s in S.doc_starts]
        rb.set_docs(S.doc_names, other)
        assert bare() == ENOTLOADED
        rep.docs_prepare()
        got, _ = _fused(rep, *d, N, S.H, ordered=True)
        _same(got, model(wlocs, woff, other), "replica, new table")
    finally:
        rep.close()
        rb.set_docs(S.doc_names, S.doc_starts)


def test_refusals_without_a_table(synth):
    """no documents, documents not prepared, and no device: refused"""
    S = synth
    L = ra.lib()
    rb = ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0)
    try:
        d = tuple(_t(np.zeros(2, np.uint64)) for _ in range(3))

        def bare():
            return L.rbg_locate_doc_hits_dev(rb.h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 2, MAXU, None, None, None, None, None, None, _stream())
        assert bare() == ENOTLOADED
        rb.set_docs(S.doc_names, S.doc_starts)
        assert bare() == ENOTLOADED
        rb.docs_prepare()
        assert bare() == 0
        assert L.rbg_locate_doc_hits_dev(None, None, None, None, 0, MAXU, None, None, None, None, None, None, None) == -3
    finally:
        rb.close()


def test_host_call(synth, handle, searched, monkeypatch):
    """rbg_doc_hits and rbg_doc_hits_locs in chunks of 1000 reads on the default path, with RBG_DOC_HITS_FUSED=0 and with RBG_DOC_HITS_CHUNK_LOCS=7 (the
    two-step path, cut into pieces): the same outputs, the model's, and the same four counters -- nothing a caller can see tells the paths apart"""
    S, rb = synth, handle
    rb.set_docs(S.doc_names, S.doc_starts)
    rb.docs_prepare()
    reads, seqs, off, wlo, whi, wk, locs = searched
    woff, wlocs = locs[MAXU]
    want = model(wlocs, woff, S.doc_starts)
    occ = np.where(whi >= wlo, whi - wlo + np.uint64(1), np.uint64(0))
    counters = [len(reads), int((occ > 0).sum()), int(occ.sum()), int(woff[-1])]
    monkeypatch.setenv("RBG_DOC_HITS_CHUNK", "1000")
    assert len(reads) > 2000
    for env in ({}, {"RBG_DOC_HITS_FUSED": "0"}, {"RBG_DOC_HITS_CHUNK_LOCS": "7"}):
        monkeypatch.delenv("RBG_DOC_HITS_FUSED", raising=False)
        monkeypatch.delenv("RBG_DOC_HITS_CHUNK_LOCS", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for with_locs in (False, True):
            rb.counters_reset()
            res = rb.doc_hits(seqs, off, MAXU, doc_locs=with_locs)
            assert rb.counters().tolist() == counters, (env, with_locs)
            assert (res[0] == wlo).all() and (res[1] == whi).all()
            got = dict(zip(OUTPUTS, res[2:]))
            assert (got.get("doc_locs") is not None) == with_locs
            _same(got, want, ("host", env, with_locs))
    # doc_reads and doc_locs accumulate into the caller's arrays
    L = ra.lib()
    N, W = len(reads), 1
    lo, hi, sets = np.zeros(N, np.uint64), np.zeros(N, np.uint64), np.zeros((N, W), np.uint64)
    ndocs = np.zeros(N, np.uint32)
    dr, dl = np.full(S.H, 5, np.uint64), np.full(S.H, 7, np.uint64)
    assert L.rbg_doc_hits_locs(rb.h, seqs.ctypes.data, off.ctypes.data, N, MAXU, lo.ctypes.data, hi.ctypes.data, sets.ctypes.data, ndocs.ctypes.data, None,
                               dr.ctypes.data, dl.ctypes.data) == 0
    assert (dr == want["doc_reads"] + np.uint64(5)).all() and (dl == want["doc_locs"] + np.uint64(7)).all() and (sets == want["sets"]).all()


def test_python_method_on_device_tensors(synth, handle, searched):
    """RowBowt.locate_doc_hits: device tensors in, tensors out"""
    S, rb = synth, handle
    rb.set_docs(S.doc_names, S.doc_starts)
    rb.docs_prepare()
    d, N = _ranges_on(rb, searched)
    woff, wlocs = searched[6][2]
    want = model(wlocs, woff, S.doc_starts)
    res = rb.locate_doc_hits(*d, max_hits=2, doc_locs=True)
    view = (np.uint64, np.uint32, np.uint32, np.uint64, np.uint64)
    _same({k: r.cpu().numpy().view(v) for k, r, v in zip(OUTPUTS, res, view)}, want, "locate_doc_hits")
    assert len(rb.locate_doc_hits(*d, order=False)) == 4
