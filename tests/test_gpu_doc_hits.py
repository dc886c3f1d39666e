"""Document hits on the device (include/rbg.h "document hits"; k_docs.hip, rbg_docdir.hpp): rbg_docs_prepare, rbg_resolve_offsets_dev[32],
rbg_doc_hits_dev[32] and the host-pointer rbg_doc_hits against the numpy model of tests/doc_hits_model.py (itself checked against the oracle in
tests/test_doc_hits_model.py) and, where a search is involved, against the oracle's locs_at_batch and resolve_offset directly.  The constants a case is
built around (the LDS limit of the table, the grid cap, the group-width thresholds) are read from the kernel's source, so that a change of a constant
fails the test instead of moving it off the boundary."""
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


def _const(name):
    src = open(os.path.join(ROOT, "rowbowt_amd", "csrc", "k_docs.hip")).read()
    m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, src)
    assert m, f"constexpr uint32_t {name} = <decimal>; not found in k_docs.hip: this file's boundary cases follow that constant"
    return int(m.group(1))


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}[a.dtype]
    return torch.from_numpy(a.view(view)).cuda()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _hits(rb, locs, loc_off, nd, skip=None, doc_reads0=None, locs32=False):
    """one rbg_doc_hits_dev[32] call on arrays built here -> {sets[N, W], ndocs, nodoc, doc_reads}; skip: the output passed as NULL (its entry is None)"""
    import torch
    L = ra.lib()
    N, W = len(loc_off) - 1, (nd + 63) // 64
    locs = np.asarray(locs, dtype=np.uint32 if locs32 else np.uint64)
    d_locs = _t(np.concatenate([locs, np.zeros(1, locs.dtype)]))
    d_off = _t(np.asarray(loc_off, dtype=np.uint64))
    out = {"sets": torch.full((max(N * W, 1),), -1, dtype=torch.int64, device="cuda"), "ndocs": torch.full((max(N, 1),), -1, dtype=torch.int32, device="cuda"),
           "nodoc": torch.full((max(N, 1),), -1, dtype=torch.int32, device="cuda"),
           "doc_reads": _t(np.zeros(nd, np.uint64) if doc_reads0 is None else np.asarray(doc_reads0, dtype=np.uint64))}
    ptr = {k: (None if k == skip else v.data_ptr()) for k, v in out.items()}
    fn = L.rbg_doc_hits_dev32 if locs32 else L.rbg_doc_hits_dev
    rc = fn(rb.h, d_locs.data_ptr(), d_off.data_ptr(), N, ptr["sets"], ptr["ndocs"], ptr["nodoc"], ptr["doc_reads"], _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    res = {"sets": out["sets"][:N * W].cpu().numpy().view(np.uint64).reshape(N, W), "ndocs": out["ndocs"][:N].cpu().numpy().view(np.uint32),
           "nodoc": out["nodoc"][:N].cpu().numpy().view(np.uint32), "doc_reads": out["doc_reads"].cpu().numpy().view(np.uint64)}
    if skip:   # the NULL output was not written: its buffer still holds what it was filled with
        fill = -1 if skip != "doc_reads" else 0
        assert doc_reads0 is not None and skip == "doc_reads" or bool((out[skip] == fill).all().item()), skip
        res[skip] = None
    return res


def _resolve(rb, locs, with_offset=True, locs32=False):
    import torch
    L = ra.lib()
    locs = np.asarray(locs, dtype=np.uint32 if locs32 else np.uint64)
    Mn = len(locs)
    d_locs = _t(np.concatenate([locs, np.zeros(1, locs.dtype)]))
    d_doc = torch.full((Mn + 1,), 7, dtype=torch.int32, device="cuda")
    d_o = torch.full((Mn + 1,), 7, dtype=torch.int64, device="cuda")
    fn = L.rbg_resolve_offsets_dev32 if locs32 else L.rbg_resolve_offsets_dev
    assert fn(rb.h, d_locs.data_ptr(), Mn, d_doc.data_ptr(), d_o.data_ptr() if with_offset else None, _stream()) == 0
    torch.cuda.synchronize()
    assert int(d_doc[Mn].item()) == 7 and int(d_o[Mn].item()) == 7   # nothing behind the M-th element
    return d_doc[:Mn].cpu().numpy().view(np.uint32), d_o[:Mn].cpu().numpy().view(np.uint64)


def _same(got, want, what):
    sets, ndocs, nodoc, doc_reads = want
    for k, w in (("sets", sets), ("ndocs", ndocs), ("nodoc", nodoc), ("doc_reads", doc_reads)):
        if got[k] is not None:
            assert got[k].shape == w.shape and (got[k] == w).all(), (what, k, np.flatnonzero((got[k] != w).reshape(len(w), -1).any(axis=1))[:5])


@pytest.fixture(scope="module")
def handle(synth):
    S = synth
    rb = ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    yield S, rb, o
    rb.close()
    o.close()


READ_SIZES = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 5000]


def _starts(S, kind):
    """the starts AS GIVEN of one table of the list"""
    rng = np.random.default_rng(17)
    if isinstance(kind, int):
        if kind == 1:
            return [0]
        s = np.sort(rng.choice(np.arange(1, S.n - 1), size=kind - 1, replace=False)).tolist()
        return [0] + s
    if kind == "first start above 0":
        return [s + 123 for s in S.doc_starts]
    assert kind == "out of order"
    s = list(S.doc_starts)
    return [s[5], s[0], s[7], s[2], s[1], s[6], s[4], s[3]]   # the last given start lies in the middle: size = s[3] + 1


def _batch(S, starts, seed):
    """reads of READ_SIZES in that order, then shuffled, an empty read first, last and between two long ones; positions: every start, start - 1, 0, size - 1,
    size, 2^64 - 1, and random ones"""
    rng = np.random.default_rng(seed)
    size = (int(starts[-1]) + 1) & MAXU
    shuffled = list(READ_SIZES)
    rng.shuffle(shuffled)
    lens = [0] + READ_SIZES + [5000, 0, 5000] + shuffled + [300, 0]
    total = sum(lens)
    special = []
    for s in starts:
        special += [int(s), (int(s) - 1) & MAXU]
    special += [0, (size - 1) & MAXU, size, MAXU, (size + 1) & MAXU, S.n - 1, S.n]
    assert len(special) < total
    locs = rng.integers(0, S.n + 40, total).astype(np.uint64)
    locs[rng.choice(total, size=len(special), replace=False)] = np.array(special, dtype=np.uint64)
    loc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return locs, loc_off


@pytest.mark.parametrize("kind", [1, 2, 64, 65, 128, 129, "lds", "lds + 1", "first start above 0", "out of order"])
def test_hand_made_batches(handle, kind, monkeypatch):
    """arrays built here straight into rbg_doc_hits_dev and rbg_resolve_offsets_dev, no search: all four outputs and doc / offset equal the model, with the
    group width chosen on the device and forced to 4, 16 and 64, and with every nullable output NULL in turn"""
    S, rb, _ = handle
    lds = _const("kDocLdsDocs")
    assert 2 * (lds + 1) < S.n, "the synthetic text is too short for a table past the LDS limit: use a longer SynthIndex"
    kind = {"lds": lds, "lds + 1": lds + 1}.get(kind, kind)
    starts = _starts(S, kind)
    nd = len(starts)
    rb.set_docs([f"d{j}" for j in range(nd)], starts)
    rb.docs_prepare()
    assert rb.doc_hits_words() == (nd + 63) // 64
    locs, loc_off = _batch(S, starts, seed=nd)
    want = M.doc_hits(locs, loc_off, starts)
    assert int(want[2].sum()) >= 1 and int(want[1].max()) >= min(nd, 2)   # some location has no document (2^64 - 1), some read meets several documents
    for group in (None, "4", "16", "64"):
        if group:
            monkeypatch.setenv("RBG_DOCS_GROUP", group)
        else:
            monkeypatch.delenv("RBG_DOCS_GROUP", raising=False)
        _same(_hits(rb, locs, loc_off, nd), want, (kind, group))
    monkeypatch.delenv("RBG_DOCS_GROUP", raising=False)
    for skip in ("sets", "ndocs", "nodoc", "doc_reads"):
        _same(_hits(rb, locs, loc_off, nd, skip=skip), want, (kind, "NULL " + skip))
    wdoc, woff = M.resolve(locs, starts)
    doc, off = _resolve(rb, locs)
    assert (doc == wdoc).all() and (off == woff).all(), kind
    doc, _ = _resolve(rb, locs, with_offset=False)
    assert (doc == wdoc).all()
    # 32-bit locations: 0xFFFFFFFF is the wrapped toehold; every other value is itself
    l32 = np.where(locs == np.uint64(MAXU), np.uint64(0xFFFFFFFF), locs).astype(np.uint32)
    _same(_hits(rb, l32, loc_off, nd, locs32=True), want, (kind, "32-bit"))
    doc, off = _resolve(rb, l32, locs32=True)
    assert (doc == wdoc).all() and (off == woff).all(), kind


def test_group_width_thresholds(handle):
    """batches whose mean number of locations lies on each side of the thresholds the launch chooses the group width by (read from the source): the
    outputs are the model's on both sides"""
    S, rb, _ = handle
    rb.set_docs(S.doc_names, S.doc_starts)
    rb.docs_prepare()
    rng = np.random.default_rng(9)
    N = 40
    for mean in (_const("kDocGroup4Mean"), _const("kDocGroup16Mean")):
        for extra in (0, 1):   # L = mean * N: the narrower width; one location more: the wider
            lens = np.full(N, mean)
            lens[:N // 2] -= min(mean, 3)
            lens[N // 2:] += min(mean, 3)
            lens[7] += extra
            assert int(lens.sum()) == mean * N + extra
            loc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
            locs = rng.integers(0, S.n, int(lens.sum())).astype(np.uint64)
            _same(_hits(rb, locs, loc_off, S.H), M.doc_hits(locs, loc_off, S.doc_starts), (mean, extra))


def test_doc_reads_accumulates(handle):
    """two calls into one d_doc_reads that was not zeroed: what it held plus both batches"""
    S, rb, _ = handle
    rb.set_docs(S.doc_names, S.doc_starts)
    rb.docs_prepare()
    rng = np.random.default_rng(10)
    held = rng.integers(1, 1000, S.H).astype(np.uint64)
    total = held.copy()
    for seed in (1, 2):
        locs, loc_off = _batch(S, S.doc_starts, seed)
        want = M.doc_hits(locs, loc_off, S.doc_starts)
        got = _hits(rb, locs, loc_off, S.H, doc_reads0=total)
        total = total + want[3]
        assert (got["doc_reads"] == total).all()
    assert (total > held).all()


def test_grid_stride_loops(handle):
    """more read groups than the largest grid holds, and more locations than its lanes: the loops go round"""
    S, rb, _ = handle
    rb.set_docs(S.doc_names, S.doc_starts)
    rb.docs_prepare()
    cap, block = _const("kDocMaxBlocks"), _const("kDocBlock")
    N = 1_000_003
    assert N > cap * block // 4 * 7 and N > cap * block   # groups of 4 lanes (a mean below kDocGroup4Mean): seven rounds; one lane per location: two
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 3, N)
    loc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    locs = rng.integers(0, S.n + 20, int(lens.sum())).astype(np.uint64)
    locs[::1001] = np.uint64(MAXU)
    assert len(locs) > cap * block
    _same(_hits(rb, locs, loc_off, S.H), M.doc_hits(locs, loc_off, S.doc_starts), "grid stride")
    wdoc, woff = M.resolve(locs, S.doc_starts)
    doc, off = _resolve(rb, locs)
    assert (doc == wdoc).all() and (off == woff).all()


def _oracle_hits(o, names, locs, loc_off):
    """the four outputs from the oracle's resolve_offset, position by position (the unique positions once)"""
    nd, W, N = len(names), (len(names) + 63) // 64, len(loc_off) - 1
    index = {n: j for j, n in enumerate(names)}
    uniq, inv = np.unique(locs, return_inverse=True)
    udoc = np.array([index.get(o.resolve_offset(int(l))[0], -1) for l in uniq], dtype=np.int64)
    doc = udoc[inv] if len(locs) else np.zeros(0, np.int64)
    sets, ndocs, nodoc, doc_reads = np.zeros((N, W), np.uint64), np.zeros(N, np.uint32), np.zeros(N, np.uint32), np.zeros(nd, np.uint64)
    for i in range(N):
        d = doc[int(loc_off[i]):int(loc_off[i + 1])]
        nodoc[i] = int((d < 0).sum())
        for j in np.unique(d[d >= 0]).tolist():
            sets[i, j // 64] |= np.uint64(1 << (j % 64))
            doc_reads[j] += np.uint64(1)
            ndocs[i] += 1
    return sets, ndocs, nodoc, doc_reads


def _device_pipeline(rb, seqs, off, max_hits, k_override=None, want32=False):
    """rbg_find_range_w_toehold_dev -> plan -> order -> fill [-> fill32] as test_device_resident_api runs them; the arrays stay on the device"""
    import torch
    L = ra.lib()
    N = len(off) - 1
    st = _stream()
    d_seqs = torch.from_numpy(np.concatenate([seqs, np.zeros((-len(seqs)) % 16 + 16, np.uint8)])).cuda()
    d_off = _t(off)
    d_lo, d_hi, d_k = (torch.empty(N, dtype=torch.int64, device="cuda") for _ in range(3))
    assert L.rbg_find_range_w_toehold_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, d_lo.data_ptr(), d_hi.data_ptr(), d_k.data_ptr(), st) == 0
    if k_override is not None:
        d_k.copy_(torch.from_numpy(k_override.view(np.int64)))
    d_loc_off = torch.empty(N + 1, dtype=torch.int64, device="cuda")
    tmp_bytes, ws_bytes = L.rbg_locate_plan_tmp_bytes(N), L.rbg_locate_order_ws_bytes(N)
    d_tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device="cuda")
    d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    assert L.rbg_locate_plan_dev(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), N, max_hits, d_loc_off.data_ptr(), d_tmp.data_ptr(), tmp_bytes, st) == 0
    total = int(d_loc_off[-1].item())
    d_locs = torch.full((max(total, 1),), -1, dtype=torch.int64, device="cuda")
    assert L.rbg_locate_order_dev(rb.h, d_k.data_ptr(), N, d_ws.data_ptr(), ws_bytes, st) == 0
    assert L.rbg_locate_fill_dev(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), d_k.data_ptr(), N, max_hits, d_loc_off.data_ptr(), d_locs.data_ptr(), d_ws.data_ptr(), st) == 0
    d_locs32 = None
    if want32:
        d_locs32 = torch.full((max(total, 1),), -1, dtype=torch.int32, device="cuda")
        assert L.rbg_locate_fill_dev32(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), d_k.data_ptr(), N, max_hits, d_loc_off.data_ptr(), d_locs32.data_ptr(),
                                       d_ws.data_ptr(), st) == 0
    torch.cuda.synchronize()
    return d_lo, d_hi, d_loc_off, d_locs, d_locs32, total


def _hits_on(rb, d_locs, d_loc_off, N, nd, locs32=False):
    import torch
    L = ra.lib()
    W = (nd + 63) // 64
    d_sets = torch.full((max(N * W, 1),), -1, dtype=torch.int64, device="cuda")
    d_nd, d_no = (torch.full((max(N, 1),), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    d_dr = torch.zeros(nd, dtype=torch.int64, device="cuda")
    fn = L.rbg_doc_hits_dev32 if locs32 else L.rbg_doc_hits_dev
    assert fn(rb.h, d_locs.data_ptr(), d_loc_off.data_ptr(), N, d_sets.data_ptr(), d_nd.data_ptr(), d_no.data_ptr(), d_dr.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    return {"sets": d_sets[:N * W].cpu().numpy().view(np.uint64).reshape(N, W), "ndocs": d_nd[:N].cpu().numpy().view(np.uint32),
            "nodoc": d_no[:N].cpu().numpy().view(np.uint32), "doc_reads": d_dr.cpu().numpy().view(np.uint64)}


def test_32_bit_locations(handle):
    """rbg_locate_fill_dev32 feeds rbg_doc_hits_dev32: the same outputs as rbg_doc_hits_dev on the 64-bit locations of the same batch, both the
    oracle's; reads whose toehold wrapped below zero (a match at text position 0; and planted on two reads of several locations, as
    test_locate_chains_in_locus_order does) are counted in nodoc by both"""
    S, rb, o = handle
    assert rb.info().pos_bytes == 4
    rb.set_docs(S.doc_names, S.doc_starts)
    rb.docs_prepare()
    reads = S.sample_reads(1500, 40, seed=21, sub_rate=0.1) + [bytes(S.text[:40]), bytes(S.text[:25]), bytes(S.text[1:30]), b"", b"ACGTN"]
    seqs, off = ra.pack_reads(reads)
    N = len(reads)
    o.set_docs(S.doc_names, S.doc_starts)
    wlo, whi, wk = o.find_range_w_toehold_batch(seqs, off, nthreads=4)
    wk = wk.copy()
    multi = np.flatnonzero(whi - wlo + 1 >= 3)[:2]
    assert len(multi) == 2
    wk[multi] = np.uint64(MAXU)
    woff, wlocs = o.locs_at_batch(wlo, whi, wk, nthreads=4)
    assert (wlocs == np.uint64(MAXU)).any(), "no wrapped toehold among the locations: the case this test is about is missing"
    d_lo, d_hi, d_loc_off, d_locs, d_locs32, total = _device_pipeline(rb, seqs, off, MAXU, k_override=wk, want32=True)
    assert total == len(wlocs) and (d_locs[:total].cpu().numpy().view(np.uint64) == wlocs).all()
    l32 = d_locs32[:total].cpu().numpy().view(np.uint32)
    assert (l32 == (wlocs & np.uint64(0xFFFFFFFF)).astype(np.uint32)).all() and (l32 == 0xFFFFFFFF).any()
    want = _oracle_hits(o, S.doc_names, wlocs, woff)
    assert int(want[2][multi].min()) >= 1   # the wrapped toeholds have no document
    _same(_hits_on(rb, d_locs, d_loc_off, N, S.H), want, "64-bit")
    _same(_hits_on(rb, d_locs32, d_loc_off, N, S.H, locs32=True), want, "32-bit")


@pytest.fixture(scope="module")
def pipeline_case(handle):
    S, rb, o = handle
    reads = [r for r in S.sample_reads(2500, 40, seed=31, sub_rate=0.1, ragged=True) if len(r) >= 2] + [bytes(S.text[:30]), b"AC", b"ACGTNACGT", b"TTTTTTTTTTTTTTTTTTTTTTTTT"]
    seqs, off = ra.pack_reads(reads)
    o.set_docs(S.doc_names, S.doc_starts)
    wlo, whi, wk = o.find_range_w_toehold_batch(seqs, off, nthreads=4)
    occ = np.where(whi >= wlo, whi - wlo + np.uint64(1), np.uint64(0))
    assert int(occ.max()) > 1000 and int((occ == 0).sum()) > 10   # counts from thousands to none
    want = {}
    for mh in (MAXU, 2, 0):
        woff, wlocs = o.locs_at_batch(wlo, whi, wk, mh, nthreads=4)
        want[mh] = (woff, wlocs, _oracle_hits(o, S.doc_names, wlocs, woff))
    return reads, seqs, off, wlo, whi, want


@pytest.mark.parametrize("max_hits", [MAXU, 2, 0])
def test_pipeline_on_the_device_and_through_the_host_call(handle, pipeline_case, max_hits, monkeypatch):
    """find_range_w_toehold_dev -> plan -> order -> fill -> rbg_doc_hits_dev against the oracle's locs_at_batch + resolve_offset; the host-pointer
    rbg_doc_hits on the same reads against the same values, in one chunk and in chunks of 1000 reads"""
    S, rb, o = handle
    reads, seqs, off, wlo, whi, want = pipeline_case
    woff, wlocs, whits = want[max_hits]
    N = len(reads)
    rb.set_docs(S.doc_names, S.doc_starts)
    rb.docs_prepare()
    d_lo, d_hi, d_loc_off, d_locs, _, total = _device_pipeline(rb, seqs, off, max_hits)
    assert (d_loc_off.cpu().numpy().view(np.uint64) == woff).all() and (d_locs[:total].cpu().numpy().view(np.uint64) == wlocs).all()
    _same(_hits_on(rb, d_locs, d_loc_off, N, S.H), whits, ("device", max_hits))
    for chunk in (None, "1000"):
        if chunk:
            monkeypatch.setenv("RBG_DOC_HITS_CHUNK", chunk)
        lo, hi, sets, ndocs, nodoc, doc_reads = rb.doc_hits(seqs, off, max_hits)
        assert (lo == wlo).all() and (hi == whi).all()
        _same({"sets": sets, "ndocs": ndocs, "nodoc": nodoc, "doc_reads": doc_reads}, whits, ("host", max_hits, chunk))
    monkeypatch.delenv("RBG_DOC_HITS_CHUNK", raising=False)


def test_pipeline_through_a_replica(handle, pipeline_case):
    """a replica on the same GPU makes its own rbg_docs_prepare from its primary's table: device calls and the host call through it; and a table set on
    the primary afterwards makes the replica's copy stale until it prepares again"""
    S, rb, o = handle
    reads, seqs, off, wlo, whi, want = pipeline_case
    woff, wlocs, whits = want[MAXU]
    N = len(reads)
    L = ra.lib()
    rb.set_docs(S.doc_names, S.doc_starts)
    rep = rb.replicate(0)
    try:
        d_lo, d_hi, d_loc_off, d_locs, _, total = _device_pipeline(rep, seqs, off, MAXU)
        assert L.rbg_doc_hits_dev(rep.h, d_locs.data_ptr(), d_loc_off.data_ptr(), N, None, None, None, None, _stream()) == ENOTLOADED   # not prepared on this handle
        rep.docs_prepare()
        _same(_hits_on(rep, d_locs, d_loc_off, N, S.H), whits, "replica, device")
        lo, hi, sets, ndocs, nodoc, doc_reads = rep.doc_hits(seqs, off, MAXU)
        assert (lo == wlo).all() and (hi == whi).all()
        _same({"sets": sets, "ndocs": ndocs, "nodoc": nodoc, "doc_reads": doc_reads}, whits, "replica, host")
        other = [s + 5 for s in S.doc_starts]
        rb.set_docs(S.doc_names, other)
        assert L.rbg_doc_hits_dev(rep.h, d_locs.data_ptr(), d_loc_off.data_ptr(), N, None, None, None, None, _stream()) == ENOTLOADED
        rep.docs_prepare()
        _same(_hits_on(rep, d_locs, d_loc_off, N, S.H), M.doc_hits(wlocs, woff, other), "replica, new table")
    finally:
        rep.close()


def test_refusals(synth):
    S = synth
    import torch
    L = ra.lib()
    rb = ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0)
    try:
        locs = np.array([0, 5, S.doc_starts[1], MAXU], dtype=np.uint64)
        loc_off = np.array([0, 3, 4], dtype=np.uint64)
        d_locs, d_off = _t(locs), _t(loc_off)
        d_doc = torch.zeros(4, dtype=torch.int32, device="cuda")
        d_nd = torch.zeros(2, dtype=torch.int32, device="cuda")
        d_doc32, d_nd32 = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")   # (the same bytes read as 32-bit locations)
        st = _stream()

        def both():
            return (L.rbg_doc_hits_dev(rb.h, d_locs.data_ptr(), d_off.data_ptr(), 2, None, d_nd.data_ptr(), None, None, st),
                    L.rbg_resolve_offsets_dev(rb.h, d_locs.data_ptr(), 4, d_doc.data_ptr(), None, st),
                    L.rbg_doc_hits_dev32(rb.h, d_locs.data_ptr(), d_off.data_ptr(), 2, None, d_nd32.data_ptr(), None, None, st),
                    L.rbg_resolve_offsets_dev32(rb.h, d_locs.data_ptr(), 4, d_doc32.data_ptr(), None, st))
        # a handle without documents
        assert both() == (ENOTLOADED,) * 4 and L.rbg_docs_prepare(rb.h) == ENOTLOADED and L.rbg_doc_hits_words(rb.h) == 0
        seqs, off = ra.pack_reads([b"ACGT"])
        out = [np.zeros(1, np.uint64) for _ in range(3)] + [np.zeros(1, np.uint32)]
        assert L.rbg_doc_hits(rb.h, seqs.ctypes.data, off.ctypes.data, 1, MAXU, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data,
                              None, None) == ENOTLOADED
        # documents, not prepared
        rb.set_docs(S.doc_names, S.doc_starts)
        assert both() == (ENOTLOADED,) * 4
        rb.docs_prepare()
        rb.docs_prepare()   # idempotent
        assert both() == (0,) * 4
        torch.cuda.synchronize()
        assert d_nd.cpu().tolist() == [2, 0] and d_doc.cpu().numpy().view(np.uint32).tolist() == [0, 0, 1, M.DOC_NONE]
        # bad arguments
        assert L.rbg_doc_hits_dev(rb.h, None, d_off.data_ptr(), 2, None, d_nd.data_ptr(), None, None, st) == EARG
        assert L.rbg_doc_hits_dev(rb.h, d_locs.data_ptr(), None, 2, None, d_nd.data_ptr(), None, None, st) == EARG
        assert L.rbg_resolve_offsets_dev(rb.h, d_locs.data_ptr(), 4, None, None, st) == EARG
        assert L.rbg_doc_hits(rb.h, seqs.ctypes.data, off.ctypes.data, 1, MAXU, None, out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data, None, None) == EARG
        # another table: stale until the next prepare, then right for the new table
        other = [0, 10, 4000]
        rb.set_docs(["x", "y", "z"], other)
        assert both() == (ENOTLOADED,) * 4
        rb.docs_prepare()
        assert both() == (0,) * 4
        torch.cuda.synchronize()
        wdoc, _ = M.resolve(locs, other)
        assert (d_doc.cpu().numpy().view(np.uint32) == wdoc).all() and d_nd.cpu().tolist() == M.doc_hits(locs, loc_off, other)[1].tolist()
        doc, offs = rb.resolve_offsets(locs)
        assert (doc == wdoc).all() and (offs == M.resolve(locs, other)[1]).all()
        # one document more than the device table holds
        many = np.arange(capi.DOCS_MAX + 1, dtype=np.uint64)
        rb.set_docs(["d"] * (capi.DOCS_MAX + 1), many)
        assert L.rbg_docs_prepare(rb.h) == EARG and both() == (ENOTLOADED,) * 4
        assert L.rbg_doc_hits(rb.h, seqs.ctypes.data, off.ctypes.data, 1, MAXU, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data,
                              None, None) == EARG
        rb.set_docs(["d"] * capi.DOCS_MAX, many[:-1])
        rb.docs_prepare()
        assert both() == (0,) * 4
        torch.cuda.synchronize()
        assert (d_doc.cpu().numpy().view(np.uint32) == M.resolve(locs, many[:-1])[0]).all()
    finally:
        rb.close()


def _host_hits(rb, seqs, off, max_hits=MAXU):
    lo, hi, sets, ndocs, nodoc, doc_reads = rb.doc_hits(seqs, off, max_hits)
    return lo, hi, {"sets": sets, "ndocs": ndocs, "nodoc": nodoc, "doc_reads": doc_reads}


@pytest.mark.parametrize("max_locs", ["1", "7", "300", "1000"])
def test_host_call_cut_into_pieces_of_bounded_locations(handle, pipeline_case, max_locs, monkeypatch):
    """rbg_doc_hits searches a chunk once and cuts its locate and reduction into pieces of at most RBG_DOC_HITS_CHUNK_LOCS locations, halving a piece that is
    over the bound down to one read (whose locations, more than the bound, are then taken whole: reads of this batch have thousands).  Whatever the cut -- one
    chunk, or chunks of 700 reads, with bounds of 1, 7, 300 and 1000 locations -- the outputs are those of the uncut call and the oracle's, and rbg_counters
    advances by exactly the same four numbers: every read searched once, every location walked once"""
    S, rb, o = handle
    reads, seqs, off, wlo, whi, want = pipeline_case
    woff, wlocs, whits = want[MAXU]
    assert int(np.diff(woff.astype(np.int64)).max()) > 1000 and int(max_locs) < int(woff[-1])   # a read alone is over every bound used here
    rb.set_docs(S.doc_names, S.doc_starts)
    rb.docs_prepare()
    monkeypatch.delenv("RBG_DOC_HITS_CHUNK", raising=False)
    monkeypatch.delenv("RBG_DOC_HITS_CHUNK_LOCS", raising=False)
    rb.counters_reset()
    lo, hi, got = _host_hits(rb, seqs, off)
    uncut = rb.counters().copy()
    assert (lo == wlo).all() and (hi == whi).all()
    _same(got, whits, "uncut")
    occ = np.where(whi >= wlo, whi - wlo + np.uint64(1), np.uint64(0))
    assert uncut.tolist() == [len(reads), int((occ > 0).sum()), int(occ.sum()), int(woff[-1])]
    for chunk in (None, "700"):
        if chunk:
            monkeypatch.setenv("RBG_DOC_HITS_CHUNK", chunk)
        monkeypatch.setenv("RBG_DOC_HITS_CHUNK_LOCS", max_locs)
        rb.counters_reset()
        lo, hi, got = _host_hits(rb, seqs, off)
        assert (lo == wlo).all() and (hi == whi).all()
        _same(got, whits, ("cut", chunk, max_locs))
        assert rb.counters().tolist() == uncut.tolist(), (chunk, max_locs)
    # a capped max_hits under a bound below it: pieces of one or two reads
    monkeypatch.setenv("RBG_DOC_HITS_CHUNK_LOCS", "3")
    lo, hi, got = _host_hits(rb, seqs, off, 2)
    _same(got, want[2][2], "max_hits 2, bound 3")


def test_grid_stride_loops_of_the_wider_groups_and_the_wide_kernel(handle, monkeypatch):
    """the loops of the 16- and 64-lane groups and of the kernel for tables above kDocLdsDocs go round too: more reads than groups of the largest grid"""
    S, rb, _ = handle
    cap, block, lds = _const("kDocMaxBlocks"), _const("kDocBlock"), _const("kDocLdsDocs")
    rng = np.random.default_rng(12)
    N = cap * block // 16 * 2 + 77                     # two rounds and a remainder of 16-lane groups; eight of 64-lane groups
    lens = rng.integers(0, 3, N)
    lens[::5000] = 70
    loc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    locs = rng.integers(0, S.n + 20, int(lens.sum())).astype(np.uint64)
    locs[::997] = np.uint64(MAXU)
    rb.set_docs(S.doc_names, S.doc_starts)
    rb.docs_prepare()
    want = M.doc_hits(locs, loc_off, S.doc_starts)
    for group in ("16", "64"):
        monkeypatch.setenv("RBG_DOCS_GROUP", group)
        assert N > cap * block // int(group)
        _same(_hits(rb, locs, loc_off, S.H), want, ("grid stride", group))
    monkeypatch.delenv("RBG_DOCS_GROUP", raising=False)
    # the wide kernel: four 64-lane groups per workgroup
    starts = _starts(S, lds + 1)
    rb.set_docs([f"d{j}" for j in range(lds + 1)], starts)
    rb.docs_prepare()
    Nw = cap * block // 64 * 2 + 5
    assert Nw > cap * block // 64
    _same(_hits(rb, locs[:int(loc_off[Nw])], loc_off[:Nw + 1], lds + 1), M.doc_hits(locs[:int(loc_off[Nw])], loc_off[:Nw + 1], starts), "grid stride, wide kernel")


def test_cpp_shim_doc_hits_and_resolve_offsets(data_dir, tmp_path, simple_reads, error_reads):
    """rowbowt_gpu.hpp doc_hits (with DocHits::hit) and the batched resolve_offsets, instantiated and run (tests/cpp/doc_hits_shim_check.cpp): an out-of-order
    table whose last given start lies in the middle, and one in order; positions at every start, start - 1, 0, size - 1, size, 2^64 - 1; against the
    oracle's locs_at_batch and resolve_offset"""
    import subprocess
    o = orc.Oracle.load(os.path.join(data_dir, "small.fa"), orc.SA)
    exe = tmp_path / "doc_hits_shim_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rowbowt_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "doc_hits_shim_check.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "rowbowt_amd"), "-lrbg", "-Wl,-rpath," + os.path.join(ROOT, "rowbowt_amd")])
    reads = [r for r in (simple_reads + error_reads) if r and b"\n" not in r][:40] + [b"AC", b"ACG", b"TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT"]
    qfile = tmp_path / "q.txt"
    qfile.write_bytes(b"\n".join(reads) + b"\n")
    seqs, off = ra.pack_reads(reads)
    wlo, whi, wk = o.find_range_w_toehold_batch(seqs, off)
    n = o.n
    for starts, max_hits in (([20000, 0, 25000, 5000, 12000], MAXU), ([0, 3000, 9000, 21000], 3), ([17, 4000], MAXU)):
        names = [f"d{j}" for j in range(len(starts))]
        o.set_docs(names, starts)
        size = starts[-1] + 1
        positions = sorted({p & MAXU for s in starts for p in (s, s - 1, s + 1)} | {0, size - 1, size, size + 1, n - 1, MAXU})
        p = subprocess.run([str(exe), os.path.join(data_dir, "small.fa"), str(qfile), str(max_hits), ",".join(map(str, starts)), ",".join(map(str, positions))],
                           capture_output=True, timeout=300)
        assert p.returncode == 0, p.stdout.decode()[-500:] + p.stderr.decode()[-2000:]
        woff, wlocs = o.locs_at_batch(wlo, whi, wk, max_hits)
        sets, ndocs, nodoc, doc_reads = _oracle_hits(o, names, wlocs, woff)
        lines = []
        for i in range(len(reads)):
            lines.append(f"read {int(wlo[i])} {int(whi[i])} {int(ndocs[i])} {int(nodoc[i])} " + " ".join(str(int(w)) for w in sets[i]))
            lines.append(" ".join(["bits"] + [str(d) for d in range(len(starts)) if (int(sets[i, d // 64]) >> (d % 64)) & 1]))
        lines.append(" ".join(["reads"] + [str(int(c)) for c in doc_reads]))
        srt = sorted(starts)
        none = 0
        for pos in positions:
            name, offs = o.resolve_offset(pos)
            if name is None:
                lines.append(f"pos {pos} none {pos} -")
                none += 1
            else:
                lines.append(f"pos {pos} {names.index(name)} {offs} {name}")
                assert offs == pos - srt[names.index(name)]
        lines.append("single 1")
        assert p.stdout.decode().splitlines() == lines, starts
        assert none >= 1 and int(ndocs.max()) >= 2
    o.close()
