"""GPU parity by EXHAUSTION (needs an MI355X): every short pattern, every text window, every row and every text position of a test-sized
index, on every layout family, against tests/text_ref.py -- the text and its suffix array, not the oracle.  The other parity files draw
samples of reads; a wrong entry in one k-mer table, one bucket edge or one phi slot is hit by a sample only by luck, and by these sweeps
always (tests/sweeps.py has the items; tests/test_text_ref.py holds the oracle to the same ones on the CPU).  All comparisons are exact
and nothing is subsampled; a failure names the configuration, the first differing pattern / row / range and how many differ."""
import contextlib
import os

import numpy as np
import pytest

import rowbowt_amd as ra
from rowbowt_amd import capi
import sweeps
from sweeps import MAXU

pytestmark = pytest.mark.gpu

SLOTS, RUNS = capi.LAYOUT_SLOTS, capi.LAYOUT_RUNS
O = capi


def _case(id_, text="synth", opts=None, env=None, packed=None, parts="ABC", expect=None, device_api=False):
    return pytest.param(dict(id=id_, text=text, opts=opts or {}, env=env or {}, packed=packed, parts=parts, expect=expect, device_api=device_api), id=id_)


def _runs(li, mask=None, recs=None, dirs=None, phi_slots=None):
    assert mask is None or li.depth_mask_kept == mask, hex(li.depth_mask_kept)
    assert recs is None or (sum(li.rec_bytes) > 0) == recs, list(li.rec_bytes)
    assert dirs is None or li.rank_directories == dirs
    assert phi_slots is None or (li.phi_slots > 0) == phi_slots
    return True


FORMAT2 = {O.OPT_POS_BYTES: 8, O.OPT_RUN_PHI: 1, O.OPT_RUN_REC: 1}        # (phi over the list of sampled positions: the structure with fillers and super counts)
UNIFORM = {O.OPT_RANK_LAYOUT: RUNS, O.OPT_RUN_PHI: 2, O.OPT_RUN_REC: 2, O.OPT_POS_BYTES: 8, O.OPT_KMER_STEPS: 8}
CROWDED = dict(text="crowded", parts="aBC")                               # sweep A's lengths 1..9, sweeps B and C in full

CASES = [
    # the slot layout (test_gpu_slots.py test_synth_all_paths)
    _case("slots-ks5-pos4", opts={O.OPT_RANK_LAYOUT: SLOTS, O.OPT_KMER_STEPS: 5, O.OPT_POS_BYTES: 4}, expect=lambda rb: rb.info().kmer_steps == 5 and rb.info().pos_bytes == 4),
    _case("slots-ks3-pos8", opts={O.OPT_RANK_LAYOUT: SLOTS, O.OPT_KMER_STEPS: 3, O.OPT_POS_BYTES: 8}, expect=lambda rb: rb.info().kmer_steps == 3 and rb.info().pos_bytes == 8),
    # the run-indexed layout (test_gpu_runs.py)
    _case("runs-default", opts={O.OPT_RANK_LAYOUT: RUNS}, device_api=True, expect=lambda rb: _runs(rb.layout_info(), mask=0x8B, recs=True, phi_slots=True)),
    _case("runs-directories-philist", opts={O.OPT_RANK_LAYOUT: RUNS, O.OPT_RUN_REC: 1, O.OPT_RUN_PHI: 1}, expect=lambda rb: _runs(rb.layout_info(), mask=0x8B, recs=False, dirs=1, phi_slots=False)),
    _case("runs-rec@deepest", opts={O.OPT_RANK_LAYOUT: RUNS, O.OPT_RUN_REC: 2, O.OPT_RUN_REC_DEPTHS: 0x80},
          expect=lambda rb: _runs(rb.layout_info(), mask=0x8B, recs=True, dirs=1) and [d for d in range(8) if rb.layout_info().rec_bytes[d]] == [7]),
    _case("runs-all-depths", opts={O.OPT_RANK_LAYOUT: RUNS, O.OPT_RUN_DEPTHS: 0xFF}, expect=lambda rb: _runs(rb.layout_info(), mask=0xFF)),
    _case("runs-sparse-0xA5", opts={O.OPT_RANK_LAYOUT: RUNS, O.OPT_RUN_DEPTHS: 0xA5, O.OPT_RUN_REC: 2}, expect=lambda rb: _runs(rb.layout_info(), mask=0xA5, recs=True)),
    _case("runs-uniform0-rec9-pos8", opts=UNIFORM, env={"RBG_RUN_UNIFORM": "0", "RBG_RUN_REC_PER": "9"}, expect=lambda rb: sum(rb.layout_info().rec_overflow) > 0),
    _case("runs-uniform1-rec9-pos8", opts=UNIFORM, env={"RBG_RUN_UNIFORM": "1", "RBG_RUN_REC_PER": "9"}, expect=lambda rb: sum(rb.layout_info().rec_overflow) > 0),
    _case("runs-format2-fillers-fine", opts={**FORMAT2, O.OPT_RANK_LAYOUT: RUNS, O.OPT_KMER_STEPS: 3, O.OPT_RUN_DEPTHS: 0x7},
          env={"RBG_RUN_FILL_SHIFT": "4", "RBG_PHI_SUPER_SHIFT": "1", "RBG_RANK_DIR_RUNS": "1", "RBG_PHI_DIR_PER": "0.5"},
          expect=lambda rb: rb.layout_info().fill_shift == 4 and sum(rb.layout_info().fillers) > 0 and rb.layout_info().phi_fillers > 0),
    _case("runs-format2-fillers-coarse", opts={**FORMAT2, O.OPT_RANK_LAYOUT: RUNS, O.OPT_KMER_STEPS: 5, O.OPT_RUN_DEPTHS: 0x1F},
          env={"RBG_RUN_FILL_SHIFT": "4", "RBG_PHI_SUPER_SHIFT": "1", "RBG_RANK_DIR_RUNS": "40", "RBG_PHI_DIR_PER": "9"},
          expect=lambda rb: rb.layout_info().fill_shift == 4 and sum(rb.layout_info().fillers) > 0 and rb.layout_info().phi_fillers > 0),
    _case("runs-ftab0", opts={O.OPT_RANK_LAYOUT: RUNS, O.OPT_FTAB_K: 0}),
    _case("runs-ftab3", opts={O.OPT_RANK_LAYOUT: RUNS, O.OPT_FTAB_K: 3}),
    _case("slots-ftab0", opts={O.OPT_RANK_LAYOUT: SLOTS, O.OPT_FTAB_K: 0}),
    # the jump table forced at K = 16 (test_gpu_jump_table.py: the probe lives in the staged byte-form walk)
    _case("runs-jump16", opts={O.OPT_RANK_LAYOUT: RUNS, O.OPT_JUMP_K: 16}, packed=0, expect=lambda rb: rb.jump_info().k == 16 and rb.jump_info().keys > 0),
    # the read forms: byte kernels and 2-bit packed reads (sweep A: B and C take no reads)
    _case("runs-default-bytes", opts={O.OPT_RANK_LAYOUT: RUNS}, packed=0, parts="A"),
    _case("runs-default-packed", opts={O.OPT_RANK_LAYOUT: RUNS}, packed=2, parts="A"),
    _case("slots-ks5-pos4-bytes", opts={O.OPT_RANK_LAYOUT: SLOTS, O.OPT_KMER_STEPS: 5}, packed=0, parts="A"),
    _case("slots-ks5-pos4-packed", opts={O.OPT_RANK_LAYOUT: SLOTS, O.OPT_KMER_STEPS: 5}, packed=2, parts="A"),
    # the crowded-bucket text (test_run_indexed_crowded_buckets): both position widths, directories and bucket records
    _case("crowded-dir-pos4", opts={O.OPT_RANK_LAYOUT: RUNS, O.OPT_RUN_REC: 1, O.OPT_POS_BYTES: 4}, **CROWDED),
    _case("crowded-dir-pos8", opts={O.OPT_RANK_LAYOUT: RUNS, O.OPT_RUN_REC: 1, O.OPT_POS_BYTES: 8}, env={"RBG_RANK_DIR_RUNS": "64"}, **CROWDED),
    _case("crowded-rec-pos4", opts={O.OPT_RANK_LAYOUT: RUNS, O.OPT_RUN_REC: 2, O.OPT_POS_BYTES: 4}, expect=lambda rb: sum(rb.layout_info().rec_overflow) > 0, **CROWDED),
    _case("crowded-rec-pos8", opts={O.OPT_RANK_LAYOUT: RUNS, O.OPT_RUN_REC: 2, O.OPT_POS_BYTES: 8}, env={"RBG_RANK_DIR_RUNS": "64", "RBG_RUN_REC_PER": "64"},
          expect=lambda rb: sum(rb.layout_info().rec_overflow) > 0, **CROWDED),
    # six symbols that are not ACGT (test_gpu_goldens.py test_random_alphabets): rank and phi, with the symbols the text holds and one it does not
    _case("sigma6-slots", text="sigma6", opts={O.OPT_RANK_LAYOUT: SLOTS}, parts="BC"),
    _case("sigma6-runs", text="sigma6", opts={O.OPT_RANK_LAYOUT: RUNS}, parts="BC"),
]

_shared = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_shared():
    yield
    _shared.clear()


def _text(name, synth):
    """the index of a text and its sweeps with what text_ref says: made once, shared by the cases, never changed"""
    if name not in _shared:
        if name == "synth":
            X = sweeps.Index(synth.text, synth.fm.sa)
        else:
            X = sweeps.Index(sweeps.crowded_text() if name == "crowded" else sweeps.alphabet_text())
        ref = X.ref
        if name == "sigma6":
            symbols = ref.symbols.tolist() + [next(c for c in range(2, 256) if ref.code[c] < 0)]
        else:
            symbols = list(b"ACGT\x01N")
        made = {"X": X, "B": sweeps.sweep_b(ref, symbols), "C": sweeps.sweep_c(ref)}
        if name != "sigma6":
            made["A"] = sweeps.sweep_a(ref, short_only=(name == "crowded"))
        assert len(made["B"][0]) == len(symbols) * (3 * X.n + len(X.heads) - 1)
        _shared[name] = made
    return _shared[name]


def _load(X, opts, env):
    saved = {k: os.environ.get(k) for k in env}
    with contextlib.ExitStack() as stack:
        for opt, value in opts.items():
            stack.enter_context(capi.default_option(opt, value))
        os.environ.update(env)
        try:
            return ra.RowBowt.from_runs(X.heads, X.lens, X.ssa, X.esa, device=0)
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _device_locate(rb, r, order, fill32):
    """sweep C's ranges through the device entry points: rbg_locate_plan_dev, (rbg_locate_order_dev,) rbg_locate_fill_dev / _dev32"""
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    L = ra.lib()
    N = len(r.lo)
    d_lo, d_hi, d_k = (torch.from_numpy(a.view(np.int64).copy()).to(dev) for a in (r.lo, r.hi, r.k))
    d_loc_off = torch.empty(N + 1, dtype=torch.int64, device=dev)
    tmp_bytes, ws_bytes = L.rbg_locate_plan_tmp_bytes(N), L.rbg_locate_order_ws_bytes(N)
    d_tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=dev)
    assert L.rbg_locate_plan_dev(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), N, r.max_hits, d_loc_off.data_ptr(), d_tmp.data_ptr(), tmp_bytes, st) == 0
    total = int(d_loc_off[-1].item())
    assert total == int(r.want_off[-1]), (r.name, total, int(r.want_off[-1]))
    d_ws = None
    if order:
        d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        assert L.rbg_locate_order_dev(rb.h, d_k.data_ptr(), N, d_ws.data_ptr(), ws_bytes, st) == 0
    d_locs = torch.full((total + 2,), -7, dtype=torch.int32 if fill32 else torch.int64, device=dev)
    fill = L.rbg_locate_fill_dev32 if fill32 else L.rbg_locate_fill_dev
    assert fill(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), d_k.data_ptr(), N, r.max_hits, d_loc_off.data_ptr(), d_locs.data_ptr(), d_ws.data_ptr() if order else None, st) == 0
    torch.cuda.synchronize()
    assert d_locs[total:].tolist() == [-7, -7], r.name                      # nothing written behind the last range
    locs = d_locs[:total].cpu().numpy()
    locs = locs.view(np.uint32).astype(np.uint64) if fill32 else locs.view(np.uint64)
    return d_loc_off.cpu().numpy().view(np.uint64), locs


# Sweeps D to G (seeds, checkpoints, marker windows, lmems) read neither the jump table (only k_runs.hip and k_jump.hip name DevIndex::jump) nor
# the packed-read option (only find_range_host_core, capi/hostpath.ipp, loads g_opt_packed_reads): these cases build the index of another case.
SEED_DUPLICATES = {"runs-jump16": "runs-default", "runs-default-bytes": "runs-default", "runs-default-packed": "runs-default",
                   "slots-ks5-pos4-bytes": "slots-ks5-pos4", "slots-ks5-pos4-packed": "slots-ks5-pos4"}
# (the four crowded-* cases: D1, D2 and D5 of a text of 637 501 symbols, 1 274 919 reads per call, the expected values made once for the four)
SEED_CASES = [c for c in CASES if c.values[0]["text"] in ("synth", "crowded") and c.values[0]["id"] not in SEED_DUPLICATES]


def _seed_sweeps(name, synth):
    """the reads of sweeps D to G over a text with what the text says, made once: the session's synthetic pangenome with its markers, all reads; the
    crowded text with sweeps.strided_markers, D1, D2 and D5 (lmems on D5)"""
    if "seeds-" + name not in _shared:
        X = _text(name, synth)["X"]
        if name == "synth":
            S = sweeps.SeedSweeps(X, synth.markers(10), sweeps.SeedItems(X))
        else:
            S = sweeps.SeedSweeps(X, sweeps.strided_markers(X, stride=sweeps.CROWDED_MARKER_STRIDE), sweeps.SeedItems(X, parts="12", lmem_windows=False))
        print("sweeps D to G on %s: expected values from the text in %.1f s: %s" % (name, S.seconds, S.assert_not_vacuous(name, two_run_windows=(name == "crowded"))))
        _shared["seeds-" + name] = S
    return _shared["seeds-" + name]


def _dev_reads(seqs, off):
    import torch
    dev = torch.device("cuda:0")
    d_seqs = torch.from_numpy(np.concatenate([seqs, np.zeros(16 + (-len(seqs)) % 16, np.uint8)])).to(dev)
    return d_seqs, torch.from_numpy(off.view(np.int64).copy()).to(dev)


class _DevicePairs:
    """rbg_greedy_seeds_plan_dev / _fill_dev and rbg_marker_seeds_plan_dev / _fill_dev behind the host calls' signatures: every output slot
    pre-filled with -1 and one spare slot given, so that a missed or a stray write shows"""

    def __init__(self, rb):
        self.rb = rb

    def get_seeds_greedy(self, seqs, off, min_length, w_sample=True):
        import torch
        d_seqs, d_off = _dev_reads(seqs, off)
        dev, N, L = d_seqs.device, len(off) - 1, ra.lib()
        st = torch.cuda.current_stream().cuda_stream
        flags = capi.SEEDS_W_SAMPLE if w_sample else 0
        tmp_bytes = int(L.rbg_greedy_seeds_tmp_bytes(N))
        d_tmp = torch.empty(max(tmp_bytes, 1), dtype=torch.uint8, device=dev)
        d_soff = torch.full((N + 1,), -1, dtype=torch.int64, device=dev)
        assert L.rbg_greedy_seeds_plan_dev(self.rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, min_length, flags, d_soff.data_ptr(), d_tmp.data_ptr(), tmp_bytes, st) == 0
        soff = d_soff.cpu().numpy().view(np.uint64)
        S = int(soff[-1])
        d_out = [torch.full((S + 1,), -1, dtype=torch.int64, device=dev) for _ in range(5)]
        assert L.rbg_greedy_seeds_fill_dev(self.rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, min_length, flags, d_soff.data_ptr(), *[t.data_ptr() for t in d_out], st) == 0
        torch.cuda.synchronize()
        cols = [t.cpu().numpy() for t in d_out]
        assert all(int(c[S]) == -1 for c in cols), "a write past the last record"
        return (soff,) + tuple(c[:S].view(np.uint64) for c in cols)

    def get_markers_greedy_seeding(self, seqs, off, wsize, max_range=MAXU, ftab_k=0):
        import torch
        d_seqs, d_off = _dev_reads(seqs, off)
        dev, N, L = d_seqs.device, len(off) - 1, ra.lib()
        st = torch.cuda.current_stream().cuda_stream
        tmp_bytes = int(L.rbg_locate_plan_tmp_bytes(N))
        d_tmp = torch.empty(max(tmp_bytes, 1), dtype=torch.uint8, device=dev)
        d_soff, d_moff = (torch.full((N + 1,), -1, dtype=torch.int64, device=dev) for _ in range(2))
        assert L.rbg_marker_seeds_plan_dev(self.rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, wsize, max_range, ftab_k, d_soff.data_ptr(), d_moff.data_ptr(),
                                           d_tmp.data_ptr(), tmp_bytes, st) == 0
        ns, nm = int(d_soff[-1].item()), int(d_moff[-1].item())
        d_rec = torch.full(((ns + 1) * 6,), -1, dtype=torch.int64, device=dev)
        d_mk = torch.full((nm + 1,), -1, dtype=torch.int64, device=dev)
        assert L.rbg_marker_seeds_fill_dev(self.rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, wsize, max_range, ftab_k, d_soff.data_ptr(), d_moff.data_ptr(),
                                           d_rec.data_ptr(), d_mk.data_ptr(), st) == 0
        torch.cuda.synchronize()
        rec, mk = d_rec.cpu().numpy(), d_mk.cpu().numpy()
        assert (rec[ns * 6:] == -1).all() and int(mk[nm]) == -1, "a write past the last record or marker"
        return d_soff.cpu().numpy().view(np.uint64), rec[:ns * 6].view(np.uint64).reshape(ns, 6), mk[:nm].view(np.uint64)


@pytest.mark.parametrize("case", SEED_CASES)
def test_seed_sweeps(synth, case):
    """sweeps D to G (tests/sweeps.py) through the host API on one index build per configuration: every seed list, longest seed, greedy location,
    checkpoint, marker window, marker seed and lmem record of the sweeps' reads against the text; on runs-default the device pairs too.  Exact,
    nothing subsampled; the configurations of SEED_DUPLICATES are left out."""
    S = _seed_sweeps(case["text"], synth)
    X = _text(case["text"], synth)["X"]
    rb = _load(X, case["opts"], case["env"])
    try:
        info = rb.info()
        cfg = "%s (n = %d, r = %d, layout %d, %d symbols per step, %d-byte positions)" % (case["id"], X.n, len(X.heads), info.rank_layout, info.kmer_steps, info.pos_bytes)
        assert info.rank_layout == case["opts"][O.OPT_RANK_LAYOUT] and info.n == X.n, cfg
        if case["expect"] is not None:
            assert case["expect"](rb) is not False, cfg
        rb.set_markers(*S.markers)
        took = sweeps.run_sweep_d(cfg, rb, S)
        if case["device_api"]:
            t = sweeps.run_sweep_d(cfg + " device pairs", _DevicePairs(rb), S, parts="df")
            took["device pairs"] = sum(v for k, v in t.items() if k != "compared")
        compared = took.pop("compared")
        assert compared["G"] > (10 ** 6 if case["text"] == "synth" else 10 ** 3) and compared["D"] > 10 ** 5 and compared["F"] > 10 ** 5 and compared["E"] > 10 ** 5, (cfg, compared)
        print("%s: seconds per sweep %s, expected records and values compared %s" % (case["id"], {k: round(v, 2) for k, v in took.items()}, compared))
    finally:
        rb.close()


@pytest.mark.parametrize("case", CASES)
def test_sweeps(synth, case):
    """sweeps A to C (tests/sweeps.py) on one index build per configuration; `parts`: A = all of sweep A, a = its lengths 1..9, B, C"""
    T = _text(case["text"], synth)
    X = T["X"]
    rb = _load(X, case["opts"], case["env"])
    try:
        info = rb.info()
        cfg = "%s (n = %d, r = %d, layout %d, %d symbols per step, %d-byte positions)" % (case["id"], X.n, len(X.heads), info.rank_layout, info.kmer_steps, info.pos_bytes)
        assert info.rank_layout == case["opts"][O.OPT_RANK_LAYOUT] and info.n == X.n, cfg
        if case["expect"] is not None:
            assert case["expect"](rb) is not False, cfg
        parts = case["parts"]
        if "A" in parts or "a" in parts:
            with capi.default_option(O.OPT_PACKED_READS, 1 if case["packed"] is None else case["packed"]):
                sweeps.run_sweep_a(cfg, rb, T["A"], min_present_9=3000)
        if "B" in parts:
            sweeps.run_sweep_b(cfg, rb, T["B"])
        if "C" in parts:
            sweeps.run_sweep_c(cfg, rb, T["C"])
            if case["device_api"]:
                for r in T["C"]:
                    for order in (False, True):
                        sweeps.check_locs(cfg + " rbg_locate_fill_dev" + (" ordered" if order else ""), r, *_device_locate(rb, r, order, False))
                    sweeps.check_locs(cfg + " rbg_locate_fill_dev32", r, *_device_locate(rb, r, True, True))   # (n < 2^32: the low words are the locations)
    finally:
        rb.close()
