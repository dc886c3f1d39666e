"""What a load decides -- layout, budget, depths kept and dropped, bucket records, ftab, jump table -- on test-sized indexes under option sets that
reach every branch of the plan (rbg_load_plan.hpp, capi/load.ipp), against the decisions recorded before the rules moved into that header:
tests/golden/load_decisions.json.  Every case fixes RBG_ASSUME_FREE_HBM_MB (and most RBG_OPT_HBM_BUDGET_MB), so nothing compared depends on the free
memory of the machine."""
import contextlib
import json
import os

import numpy as np
import pytest

import rowbowt_amd as ra
from rowbowt_amd import capi
from gpu_common import _random_run_index

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "load_decisions.json")
FREE_MB = "65536"   # the free HBM every case plans with unless it names another (a quarter of it: 16 GB, room for anything here)

# name -> (index, RBG_ASSUME_FREE_HBM_MB, {option: value}); the branch each one is there for is its name
CASES = {
    # the synthetic pangenome of the `synth` fixture (n = 3.2e4): its slot tables of five symbols are some 100 MB of 64 KB-aligned arrays
    "slots": ("synth", FREE_MB, {capi.OPT_HBM_BUDGET_MB: 1 << 12}),
    "runs_by_request": ("synth", FREE_MB, {capi.OPT_RANK_LAYOUT: capi.LAYOUT_RUNS, capi.OPT_HBM_BUDGET_MB: 1 << 12}),
    "auto_runs_from_options_for": ("synth", FREE_MB, {capi.OPT_HBM_BUDGET_MB: 1}),
    "second_look_in_upload": ("synth", FREE_MB, {capi.OPT_HBM_BUDGET_MB: 8}),
    "slot_level_dropped": ("synth", FREE_MB, {capi.OPT_RANK_LAYOUT: capi.LAYOUT_PREFER_SLOTS, capi.OPT_HBM_BUDGET_MB: 8}),
    "deepest_dropped": ("synth", FREE_MB, {capi.OPT_RANK_LAYOUT: capi.LAYOUT_PREFER_SLOTS, capi.OPT_HBM_BUDGET_MB: 2}),
    "jump_table_built": ("synth", FREE_MB, {capi.OPT_RANK_LAYOUT: capi.LAYOUT_RUNS, capi.OPT_HBM_BUDGET_MB: 1 << 12, capi.OPT_JUMP_K: 20}),
    # a million runs over n = 1e8 (the builder of test_gpu_runs.py's budget tests)
    "budget_raised_depth_capped": ("million", "200", {capi.OPT_FTAB_K: 0}),
    "budget_given_not_raised": ("million", "200", {capi.OPT_FTAB_K: 0, capi.OPT_HBM_BUDGET_MB: 60}),
    "middle_depth_dropped": ("million", FREE_MB, {capi.OPT_RANK_LAYOUT: capi.LAYOUT_RUNS, capi.OPT_FTAB_K: 0, capi.OPT_KMER_STEPS: 5, capi.OPT_RUN_DEPTHS: 0x1F,
                                                  capi.OPT_RUN_PHI: 1, capi.OPT_RUN_REC: 1, capi.OPT_HBM_BUDGET_MB: 110}),
    # (slot tables of a depth the budget cannot hold are not composed; those composed get wider buckets, then go)
    "slot_widening": ("million", FREE_MB, {capi.OPT_RANK_LAYOUT: capi.LAYOUT_PREFER_SLOTS, capi.OPT_FTAB_K: 0, capi.OPT_HBM_BUDGET_MB: 200}),
    "ends_only": ("million", FREE_MB, {capi.OPT_RANK_LAYOUT: capi.LAYOUT_RUNS, capi.OPT_FTAB_K: 0, capi.OPT_KMER_STEPS: 5, capi.OPT_HBM_BUDGET_MB: 240}),
    "jump_table_declined": ("million", FREE_MB, {capi.OPT_RANK_LAYOUT: capi.LAYOUT_RUNS, capi.OPT_FTAB_K: 0, capi.OPT_KMER_STEPS: 5, capi.OPT_JUMP_K: 32,
                                                 capi.OPT_HBM_BUDGET_MB: 120}),
}


def decide(arrays, free_mb, opts):
    """one load under the options; the machine-independent fields of rbg_info, rbg_layout_info and rbg_jump_info"""
    heads, lens, ssa, esa = arrays
    os.environ["RBG_ASSUME_FREE_HBM_MB"] = free_mb
    try:
        with contextlib.ExitStack() as st:
            for opt, value in opts.items():
                st.enter_context(capi.default_option(opt, value))
            rb = ra.RowBowt.from_runs(heads, lens, ssa, esa, device=0)
    finally:
        del os.environ["RBG_ASSUME_FREE_HBM_MB"]
    info, li, ji = rb.info(), rb.layout_info(), rb.jump_info()
    rb.close()
    return {"layout": int(info.rank_layout), "kmer_steps": int(info.kmer_steps), "kmer_steps_requested": int(info.kmer_steps_requested),
            "hbm_free_at_load": int(info.hbm_free_at_load), "hbm_budget": int(info.hbm_budget), "budget_raised": int(li.budget_raised),
            "depth_mask_asked": int(li.depth_mask_asked), "depth_mask_kept": int(li.depth_mask_kept), "depths_dropped_budget": int(li.depths_dropped_budget),
            "depths_composed": int(li.depths_composed), "rec_bytes": [int(x) for x in li.rec_bytes], "phi_slots": int(li.phi_slots),
            "info_phi_slots": int(info.phi_slots), "hbm_bytes": int(info.hbm_bytes), "ftab_k": int(info.ftab_k), "jump_k": int(ji.k), "jump_bytes": int(ji.bytes)}


@pytest.fixture(scope="module")
def million():
    heads, lens, ssa, esa, _n = _random_run_index(np.random.default_rng(43), 1_000_000, 200)
    return heads, lens, ssa, esa


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_load_decisions_are_the_recorded_ones(synth, million, golden, name):
    index, free_mb, opts = CASES[name]
    arrays = (synth.heads, synth.lens, synth.ssa, synth.esa) if index == "synth" else million
    got = decide(arrays, free_mb, opts)
    assert got == golden[name], {k: (got[k], golden[name].get(k)) for k in got if got[k] != golden[name].get(k)}
