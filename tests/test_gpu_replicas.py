"""Replicas (rbg_replicate, capi/replicas.ipp) of every index form, with everything attached before the copy: the invariant of the re-pointed records
(rbg_reloc_check.hpp, reported by rbg_replica_pointer_check), the load's decisions as rbg_info / rbg_layout_info / rbg_jump_info report them, and every
query family on the replica against the oracle and the Python models (needs an MI355X; one GPU is enough -- a replica on the primary's device has other
addresses, so a pointer nobody re-pointed, or one re-pointed to nullptr because its array was never tracked, shows in the check although every answer
would still be right)."""
import contextlib
import os
import re

import numpy as np
import pytest

import golden_values as G
import orc
import rowbowt_amd as ra
from rowbowt_amd import capi
from gpu_common import ROOT, _check_marker_seeds, _run_indexed_checks, _with_layout, split
from lmem_model import lmem_records
from rb_locs_model import loc_markers, markers_at_loc
from seeds_model import seeds_greedy, toehold_chkpnts
from test_gpu_loc_markers import _arrays, _grid_runs
from test_gpu_seeds_list import _lists
from test_rb_locs_model import text_oracle

pytestmark = pytest.mark.gpu
MAXU = G.MAXU
JUMP_K = 16   # (a K of test_gpu_jump_table.py on this fixture)


def _dev_index_pointer_fields():
    """the pointer members of struct DevIndex, read from rbg_dev.h: a member added there is a member some form below has to make non-null"""
    src = open(os.path.join(ROOT, "rowbowt_amd", "csrc", "rbg_dev.h")).read()
    body = src[src.index("struct DevIndex {"):]
    body = body[:body.index("\n};")]
    body = re.sub(r"//[^\n]*", "", body)
    fields = []
    for stmt in body.split(";"):
        if "*" in stmt:
            fields += re.findall(r"\*\s*(\w+)", stmt)
    return set(fields)


COMMON = {"syms", "counters", "lut", "lut2", "mk_start", "mk_end", "mk_off", "mk_vals", "mk_bucket", "mk_rec",
          "tmk_start", "tmk_end", "tmk_off", "tmk_vals", "tmk_bucket", "tmk_rec", "order_docs", "ftab", "phi_ent"}
RUNS = {"run_ent2", "run_samp", "run_tabs2", "run_hot"}
# name -> (layout, default options, environment of the load, the DevIndex pointers the form exists for -- beside COMMON)
FORMS = {
    "slots4": (capi.LAYOUT_SLOTS, {capi.OPT_RANK_BUCKET_SHIFT: 8}, {},       # (256-row buckets: hundreds of them overflow on this index and get dense tables)
               {"pairs", "triples", "quads", "quints", "dense", "phi_slots", "phi_ord"}),
    "slots8": (capi.LAYOUT_SLOTS, {capi.OPT_POS_BYTES: 8}, {}, {"pairs", "triples", "quads", "quints", "phi_slots", "phi_ord"}),
    "runs4_rec_list_jump": (capi.LAYOUT_RUNS, {capi.OPT_RUN_REC: 2, capi.OPT_RUN_PHI: 1, capi.OPT_JUMP_K: JUMP_K}, {}, RUNS | {"jump", "run_rec2", "phi_dir"}),
    "runs8_phi_slots": (capi.LAYOUT_RUNS, {capi.OPT_POS_BYTES: 8, capi.OPT_RUN_PHI: 2}, {}, RUNS | {"phi_slots", "phi_ord"}),
    "runs8_fillers_super": (capi.LAYOUT_RUNS, {capi.OPT_POS_BYTES: 8, capi.OPT_KMER_STEPS: 5, capi.OPT_RUN_PHI: 1, capi.OPT_RUN_REC: 2},
                            {"RBG_RUN_FILL_SHIFT": "6", "RBG_PHI_SUPER_SHIFT": "2"}, RUNS | {"run_rec2", "phi_dir", "phi_super"}),
    "runs4_directories": (capi.LAYOUT_RUNS, {capi.OPT_RUN_REC: 1}, {}, RUNS | {"run_dir2"}),
}
# per-handle by their documentation (include/rbg.h): where the handle lives and what was free there when it was made
INFO_PER_HANDLE = {"device", "hbm_free_at_load"}


def test_forms_cover_every_pointer_of_dev_index():
    """the union over the forms of the fields each one is REQUIRED to hold non-null (test_replica_of_every_form asserts the requirement on the device) is every
    pointer member struct DevIndex has"""
    union = set(COMMON)
    for _layout, _opts, _env, need in FORMS.values():
        union |= need
    assert union == _dev_index_pointer_fields()


@contextlib.contextmanager
def _environ(env):
    prev = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in prev.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _primary(S, form):
    """the form's index on device 0 with everything attached: SA-row markers, the text-position table, the documents under the locus order"""
    layout, opts, env, _need = FORMS[form]
    with contextlib.ExitStack() as st:
        for opt, v in opts.items():
            st.enter_context(capi.default_option(opt, v))
        st.enter_context(_environ(env))
        rb = _with_layout(layout, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    rb.set_markers(*S.markers(wsize=10))
    rb.set_text_markers(*_arrays(_grid_runs(S.n)))
    with _environ({"RBG_LOCATE_ORDER": "locus"}):
        rb.set_docs(S.doc_names, S.doc_starts)
    return rb


def _fields_from_info(info, li, ji):
    """DevIndex pointer -> how many of them the load's own report says are non-null (arrays per k-mer depth count once per kept depth): what
    rbg_replica_pointer_check must have recognised, by rbg_dev.h and the upload code"""
    f = {k: 1 for k in ("syms", "counters", "lut")}
    if info.kmer_symbols >= 2 or info.rank_layout == capi.LAYOUT_RUNS:
        f["lut2"] = 1
    if info.has_markers and info.marker_runs:
        f.update({k: 1 for k in ("mk_start", "mk_end", "mk_off", "mk_vals", "mk_bucket", "mk_rec")})
    f.update({k: 1 for k in ("tmk_start", "tmk_end", "tmk_off", "tmk_vals", "tmk_bucket", "tmk_rec")})   # (set by _primary; no info field reports it)
    if info.has_docs:
        f["order_docs"] = 1
    if info.ftab_k:
        f["ftab"] = 1
    if info.has_tsa:
        f["phi_ent"] = 1
    if info.rank_layout == capi.LAYOUT_SLOTS:
        for d, name in ((2, "pairs"), (3, "triples"), (4, "quads"), (5, "quints")):
            if info.kmer_steps >= d:
                f[name] = 1
        if info.rank_slots_overflow:
            f["dense"] = 1
        if info.phi_slots:
            f["phi_slots"] = f["phi_ord"] = 1
    else:
        kept = [d for d in range(capi.MAX_KMER_DEPTH) if li.depth_mask_kept >> d & 1]
        f["run_ent2"] = len(kept)
        f["run_samp"] = len(kept) if info.has_tsa else 0
        f["run_rec2"] = sum(1 for d in kept if li.rec_bytes[d])
        f["run_dir2"] = sum(1 for d in kept if li.dir_bytes[d])
        assert f["run_rec2"] + f["run_dir2"] == len(kept)
        f["run_tabs2"] = f["run_hot"] = 1
        if li.phi_slots:
            f["phi_slots"] = f["phi_ord"] = 1
        else:
            f["phi_dir"] = 1
            if info.pos_bytes == 8:
                f["phi_super"] = 1
        if ji.k:
            f["jump"] = 1
    return {k: v for k, v in f.items() if v}


def _same_struct(a, b, skip=()):
    for name, _t in a._fields_:
        if name in skip:
            continue
        va, vb = getattr(a, name), getattr(b, name)
        if hasattr(va, "__len__"):
            va, vb = list(va), list(vb)
        assert va == vb, (type(a).__name__, name, va, vb)


@pytest.fixture(scope="module")
def ref(synth):
    """the reads of every family and what the oracle and the models say about them, computed once; the same for every form"""
    S = synth
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    o.set_markers(*S.markers(wsize=10))
    o.set_docs(S.doc_names, S.doc_starts)
    ot = text_oracle(_grid_runs(S.n))
    R = type("Ref", (), {})()
    R.S, R.o, R.ot = S, o, ot
    R.reads = ([S.text[:30].tobytes(), S.text[:100].tobytes()] + S.sample_reads(200, 70, seed=77, sub_rate=0.2, ragged=True) + S.sample_reads(60, 100, seed=5, sub_rate=0.0) +
               [b"", b"ACGTN", b"N", b"acgt", S.text[:300].tobytes(), S.text[-30:].tobytes(), S.text[-31:-1].tobytes()])
    R.seqs, R.off = ra.pack_reads(R.reads)
    R.lo, R.hi, R.k = o.find_range_w_toehold_batch(R.seqs, R.off)
    # the text's first 30 symbols, whose toehold wraps below zero on the way (the search steps left of position 0 of every haplotype but the first): found in
    # every haplotype, position 0 among them; and the first 100, which only position 0 has
    assert int(R.hi[0] - R.lo[0]) == S.H - 1 and 0 in o.locs_at(int(R.lo[0]), int(R.hi[0]), int(R.k[0])) and (int(R.lo[1]), int(R.hi[1]), int(R.k[1])) == (int(R.lo[0]), int(R.lo[0]), 0)
    assert 2 * int((R.hi >= R.lo).sum()) > len(R.reads)
    R.locs = {mh: o.locs_at_batch(R.lo, R.hi, R.k, mh) for mh in (MAXU, 3, 0)}
    assert len(R.locs[MAXU][1]) > len(R.locs[3][1]) > 0 == len(R.locs[0][1])
    rng = np.random.default_rng(3)
    R.lf_lo = rng.integers(0, S.n, 200).astype(np.uint64)
    R.lf_hi = np.minimum(R.lf_lo + rng.integers(0, 50, 200).astype(np.uint64), np.uint64(S.n - 1))
    R.lf_c = rng.choice(np.frombuffer(b"ACGT\x01N", dtype=np.uint8), 200)
    R.lf = [o.LF(int(a), int(b), int(c)) for a, b, c in zip(R.lf_lo, R.lf_hi, R.lf_c)]
    R.markers_at = [o.markers_at(int(a), int(b)) for a, b in zip(R.lo, R.hi)]
    assert sum(1 for m in R.markers_at if m) > 20
    R.sub = R.reads[:120] + R.reads[-7:]
    R.w_markers = {wm: [o.find_range_w_markers(q, *wm) for q in R.sub] for wm in ((10, MAXU), (7, 4))}
    R.small = R.reads[:50] + R.reads[-7:]
    R.lmems = {p: [lmem_records(o, q, *p) for q in R.small] for p in ((10, 1000, 0), (19, 1000, 5))}
    assert sum(len(m[4]) for w in R.lmems[(10, 1000, 0)] for m in w) > 20
    R.seeds = {(ml, ws): [seeds_greedy(o, q, ml, ws) for q in R.sub] for ml in (10, 21) for ws in (True, False)}
    assert sum(len(w) for w in R.seeds[(10, True)]) > 60 and any(len(w) > 1 for w in R.seeds[(10, True)])
    R.chk = {w: [toehold_chkpnts(o, q, w) for q in R.sub] for w in (3, 19)}
    assert sum(len(w) for w in R.chk[19]) > 50
    R.greedy = {mh: [o.greedy_locate(q, 10, mh)[0] for q in R.sub] for mh in (MAXU, 3)}
    R.loc_markers = {mh: [loc_markers(o, ot, q, 10, mh) for q in R.sub] for mh in (MAXU, 3)}
    assert sum(1 for w in R.loc_markers[MAXU] if w[1]) > 40
    # markers at given locations: the located ones of the first family, under their reads' lengths
    loc_off, locs = R.locs[MAXU]
    R.at_locs = []
    for i in range(len(R.reads)):
        got = []
        for l in locs[int(loc_off[i]):int(loc_off[i + 1])]:
            got += markers_at_loc(ot, int(l), int(R.off[i + 1] - R.off[i]))
        R.at_locs.append(got)
    assert sum(1 for w in R.at_locs if w) > 40
    R.names = [b"r%d" % i for i in range(len(R.reads))]
    yield R
    o.close()
    ot.close()


def _answers(rb, R):
    """every query family on `rb` against the shared reference"""
    o = R.o
    lo, hi, k = rb.find_range_w_toehold(R.seqs, R.off)
    assert (lo == R.lo).all() and (hi == R.hi).all() and (k == R.k).all()
    lo1, hi1 = rb.find_range(R.seqs, R.off)
    assert (lo1 == R.lo).all() and (hi1 == R.hi).all()
    cnt = rb.count(R.seqs, R.off)
    assert (cnt == np.where(R.hi >= R.lo, R.hi - R.lo + np.uint64(1), np.uint64(0))).all()
    for mh, (woff, wlocs) in R.locs.items():            # (reads 0 and 1 sit at the text's start: on the locus order their chains go through k[i])
        loc_off, locs = rb.locs_at(lo, hi, k, mh)
        assert (loc_off == woff).all() and (locs == wlocs).all(), mh
    nlo, nhi = rb.LF(R.lf_lo, R.lf_hi, R.lf_c)
    assert [(int(a), int(b)) for a, b in zip(nlo, nhi)] == R.lf
    mk_off, mk = rb.markers_at(lo, hi)
    assert split(mk_off, mk) == R.markers_at
    s3, o3 = ra.pack_reads(R.sub)
    for (wsize, max_range), want in R.w_markers.items():
        lo3, hi3, mk_off3, mk3 = rb.find_range_w_markers(s3, o3, wsize, max_range)
        got3 = split(mk_off3, mk3)
        for i, ((wl, wh), wm) in enumerate(want):
            assert (int(lo3[i]), int(hi3[i])) == (wl, wh) and got3[i] == wm, (i, wsize)
    nseed, nmk = _check_marker_seeds(rb, o, R.sub, 10, 1000)
    assert nseed > 60 and nmk > 20
    _check_marker_seeds(rb, o, R.small, 10, 1000, ftab_k=3)
    s4, o4 = ra.pack_reads(R.small)
    for (wsize, max_range, K), want in R.lmems.items():
        seed_off, seeds, mkv = rb.get_markers_lmems(s4, o4, wsize, max_range, K)
        assert (seed_off == o4).all()
        for i, w in enumerate(want):
            got = seeds[int(seed_off[i]):int(seed_off[i + 1])]
            assert [(int(g[0]), int(g[1]), int(g[2]), int(g[3]), mkv[int(g[4]):int(g[5])].tolist()) for g in got] == [tuple(x) for x in w], (i, wsize, K)
    for (min_length, w_sample), want in R.seeds.items():
        assert _lists(rb.get_seeds_greedy(s3, o3, min_length, w_sample)) == want, (min_length, w_sample)
    for wsize, want in R.chk.items():
        assert _lists(rb.find_range_w_toehold_chkpnts(s3, o3, wsize)) == want, wsize
    for mh in (MAXU, 3):
        goff, glocs = rb.find_locs_greedy_seeding(s3, o3, 10, mh)
        assert split(goff, glocs) == R.greedy[mh], mh
        loc_off, locs, mk_off, mk = rb.find_loc_markers_greedy_seeding(s3, o3, 10, mh)
        assert split(loc_off, locs) == [w[0] for w in R.loc_markers[mh]] and split(mk_off, mk) == [w[1] for w in R.loc_markers[mh]], mh
    mk_off, mk = rb.markers_at_locs(R.locs[MAXU][1], R.locs[MAXU][0], R.off)
    assert split(mk_off, mk) == R.at_locs


def _report_tally_text(rb, R):
    """the bytes of the report (records and text), of a tally made on `rb` and of the rb_align text (their models: test_gpu_report.py, test_gpu_tally.py,
    test_gpu_text_writers.py; here the primary's bytes on the same input are the reference)"""
    out = []
    for kw in (dict(wsize=10, max_range=1000), dict(wsize=10, max_range=1000, lmem=True, ftab_k=5), dict(wsize=10, best_strand=True, clear_identical=True)):
        p = capi.report_params(read_len=70, **kw)
        seed_off, recs, mk = rb.markers_report(R.seqs, R.off, p)
        out += [seed_off.tobytes(), recs.tobytes(), mk.tobytes(), rb.markers_report_text(R.seqs, R.off, R.names, p)]
        t = capi.Tally(rb, 0)
        try:
            rb.markers_tally(R.seqs, R.off, p, None, t)
            rb.markers_tally(R.seqs[:int(R.off[100])], R.off[:101], p, None, t)    # (accumulates in the table on this handle's device)
            out.append(t.export().tobytes())
        finally:
            t.close()
    lo, hi, k = R.lo, R.hi, R.k
    for with_locs, markers, mh in ((True, False, MAXU), (True, True, 3), (False, True, MAXU)):
        out.append(rb.align_text(lo, hi, k if with_locs else None, R.names, mh, markers=markers))
    return out


@pytest.mark.parametrize("form", list(FORMS))
def test_replica_of_every_form(ref, form):
    """Per form: the pointer check of the replica is clean and has recognised exactly the pointers the load's own report says the form holds -- among them the
    ones the form exists for (FORMS; test_forms_cover_every_pointer_of_dev_index: together, all of DevIndex); rbg_info, rbg_layout_info and rbg_jump_info equal
    the primary's field for field except the per-handle ones; the replica answers every query family as the oracle and the models do, its report, tally and
    text are the primary's byte for byte; a batch sharded over primary and two replicas is answered whole, the device counters summing to it."""
    import torch
    R, S = ref, ref.S
    rb = _primary(S, form)
    reps = []
    try:
        info, li, ji = rb.info(), rb.layout_info(), rb.jump_info()
        layout, opts, _env, need = FORMS[form]
        assert info.rank_layout == layout and info.pos_bytes == (opts.get(capi.OPT_POS_BYTES) or 4) and info.has_markers and info.has_docs and info.ftab_k > 0
        if "jump" in need:
            assert ji.k == JUMP_K and ji.keys > 0
        if "phi_super" in need:
            assert li.fill_shift == 6 and sum(li.fillers) > 0 and li.phi_fillers > 0
        fields = _fields_from_info(info, li, ji)
        assert (COMMON | need) <= set(fields), sorted((COMMON | need) - set(fields))
        print(f"{form}: DevIndex pointers non-null: " + " ".join(f"{k}x{v}" if v > 1 else k for k, v in sorted(fields.items())))
        ndev = torch.cuda.device_count()
        reps = [rb.replicate(1 if ndev > 1 else 0), rb.replicate(0)]
        with pytest.raises(ra.RbgError):
            rb.replica_pointer_check()                 # a primary was built, not copied
        for rep in reps:
            chk = rep.replica_pointer_check()
            print(f"{form}: {chk}")
            assert chk["dev_violations"] == 0 and chk["table_violations"] == 0, chk
            assert chk["dev_pointers"] == sum(fields.values()), (chk, fields)
            # the DevSym records of the slot layout: {ent, samp, slots, ord} of every symbol and k-mer table; the run-indexed layout has no such records
            ntab = info.sigma + sum(info.kmer_symbols ** d for d in range(2, info.kmer_steps + 1))
            assert chk["table_pointers"] == (4 * ntab if layout == capi.LAYOUT_SLOTS else 0), (chk, ntab)
            _same_struct(rep.info(), info, INFO_PER_HANDLE)
            _same_struct(rep.layout_info(), li)
            _same_struct(rep.jump_info(), ji)
        rep = reps[0]
        _answers(rep, R)
        assert _report_tally_text(rep, R) == _report_tally_text(rb, R)
        # sharded over the primary and both replicas
        for h in [rb] + reps:
            h.counters_reset()
        lo2, hi2, k2 = capi.find_range_sharded([rb] + reps, R.seqs, R.off, toehold=True)
        assert (lo2 == R.lo).all() and (hi2 == R.hi).all() and (k2 == R.k).all()
        tot = sum(h.counters().astype(np.int64) for h in [rb] + reps)
        assert tot[0] == len(R.reads) and tot[1] == int((R.hi >= R.lo).sum())
        if form == "runs4_rec_list_jump":
            _run_indexed_checks(S, reps.pop(), markers_attached=True)     # (closes the replica it is given)
    finally:
        for rep in reps:
            rep.close()
        rb.close()


@pytest.mark.parametrize("layout", [capi.LAYOUT_RUNS, capi.LAYOUT_SLOTS])
def test_documents_attached_twice_then_replicated(ref, layout):
    """rbg_set_docs a second time gives the first table's device array back: hbm_bytes is what a handle that only ever had the second table reports (and what
    a handle without an eligible table reports after a one-document table made the order ineligible), the replica copies no stale array, its pointer check
    is clean and its locations are the oracle's."""
    R, S = ref, ref.S
    load = lambda: _with_layout(layout, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    other = (["a", "b", "c"], [0, 1000, 9000])
    with _environ({"RBG_LOCATE_ORDER": "locus"}):
        fresh, rb = load(), load()
        rep = None
        try:
            none = int(rb.info().hbm_bytes)
            assert int(fresh.info().hbm_bytes) == none
            fresh.set_docs(S.doc_names, S.doc_starts)
            want = int(fresh.info().hbm_bytes)
            assert want > none                                  # the locus order's array is counted
            rb.set_docs(*other)
            assert int(rb.info().hbm_bytes) > none
            rb.set_docs(["one"], [0])                           # one document: no locus order, and the array of the table before is given back
            assert int(rb.info().hbm_bytes) == none
            rb.set_docs(*other)
            rb.set_docs(S.doc_names, S.doc_starts)
            assert int(rb.info().hbm_bytes) == want
            rep = rb.replicate(0)
            assert int(rep.info().hbm_bytes) == want
            chk = rep.replica_pointer_check()
            assert chk["dev_violations"] == 0 and chk["table_violations"] == 0 and chk["dev_pointers"] > 0, chk
            for h in (rep, rb):
                for mh, (woff, wlocs) in R.locs.items():
                    loc_off, locs = h.locs_at(R.lo, R.hi, R.k, mh)
                    assert (loc_off == woff).all() and (locs == wlocs).all(), mh
        finally:
            if rep is not None:
                rep.close()
            rb.close()
            fresh.close()
