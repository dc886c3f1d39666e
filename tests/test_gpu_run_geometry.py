"""What a load of the run-indexed layout BUILDS -- entries and fillers per depth, directory or record bytes and their overflow, the uniform geometry of the
deepest depth, phi as slots or as list + directory, the replica's bytes -- on test-sized indexes under switches that reach every branch of
capi/upload_runs.ipp upload_tables_runs2 and of the geometry rules in rbg_load_plan.hpp, against what the same loads built before that function was cut
into steps: tests/golden/run_geometry.json.  Every case fixes RBG_ASSUME_FREE_HBM_MB and RBG_OPT_HBM_BUDGET_MB, so nothing compared depends on the free
memory of the machine.  The RBG_VERBOSE lines about "uniform directories" are compared too: they carry the shift, the stride and the overflow counts of a
decision no info struct exposes."""
import contextlib
import json
import os
import re
import sys
import tempfile

import numpy as np
import pytest

import rowbowt_amd as ra
from rowbowt_amd import capi

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_geometry.json")
FREE_MB = "65536"
O = capi
RUNS = {O.OPT_RANK_LAYOUT: O.LAYOUT_RUNS, O.OPT_HBM_BUDGET_MB: 1 << 12}   # (4 GB: room for every record and slot of these indexes -- the automatic rules decide)
K5, K6, K8, POS8 = {O.OPT_KMER_STEPS: 5}, {O.OPT_KMER_STEPS: 6}, {O.OPT_KMER_STEPS: 8}, {O.OPT_POS_BYTES: 8}
DIRS, RECS, LIST, SLOTS = {O.OPT_RUN_REC: 1}, {O.OPT_RUN_REC: 2}, {O.OPT_RUN_PHI: 1}, {O.OPT_RUN_PHI: 2}
FILL = {"RBG_RUN_FILL_SHIFT": "5", "RBG_PHI_SUPER_SHIFT": "3", "RBG_RANK_DIR_RUNS": "40", "RBG_PHI_DIR_PER": "9"}

# name -> (index, {option: value}, {environment switch: value}); the branch each one is there for is its name
CASES = {
    "directories_pos4": ("synth", {**RUNS, **K5, **DIRS, **LIST}, {}),
    "directories_pos8": ("synth", {**RUNS, **K5, **DIRS, **LIST, **POS8}, {}),
    "records_pos4": ("synth", {**RUNS, **K5, **RECS, **LIST}, {}),
    "records_pos8_overflowing": ("synth", {**RUNS, **K5, **RECS, **LIST, **POS8}, {"RBG_RUN_REC_PER": "9"}),
    "records_deepest_depth_only": ("synth", {**RUNS, **K5, **RECS, **LIST, O.OPT_RUN_REC_DEPTHS: 1 << 4}, {}),
    "phi_slots_pos4": ("synth", {**RUNS, **K5, **DIRS, **SLOTS}, {}),
    "phi_slots_pos8_packed": ("synth", {**RUNS, **K5, **DIRS, **SLOTS, **POS8}, {}),
    # n / r >= 128: the slot shift is 7, beyond what a packed slot holds
    "phi_slots_pos8_not_packed": ("repeats", {**RUNS, **K5, **DIRS, **SLOTS, **POS8}, {}),
    "uniform_forced": ("synth", {**RUNS, **K8, **RECS, **SLOTS, **POS8}, {"RBG_RUN_UNIFORM": "1"}),
    "uniform_forbidden": ("synth", {**RUNS, **K8, **RECS, **SLOTS, **POS8}, {"RBG_RUN_UNIFORM": "0"}),
    "uniform_unset": ("synth", {**RUNS, **K8, **RECS, **SLOTS, **POS8}, {}),
    "uniform_unset_pos4": ("synth", {**RUNS, **K8, **RECS, **SLOTS}, {}),
    # More than one uniform record in 256 overflows: the uniform geometry is measured against the tables' own shifts.  No depth of the synthetic pangenome
    # beyond the fifth has a table of twelve entries; random bases have hundreds at depth 6.  At 16 entries per bucket the tables' own buckets are as wide
    # as the uniform ones and overflow as often: uniform stays.  At 9 the fuller tables get buckets of their own: 6 overflow against 402, the tables keep theirs.
    "uniform_compared_stays": ("random", {**RUNS, **K6, **RECS, **SLOTS, **POS8}, {"RBG_RUN_REC_PER": "16"}),
    "uniform_compared_tables_keep_own_shifts": ("random", {**RUNS, **K6, **RECS, **SLOTS, **POS8}, {"RBG_RUN_REC_PER": "9"}),
    "uniform_compared_tables_keep_own_shifts_pos4": ("random", {**RUNS, **K6, **RECS, **SLOTS}, {"RBG_RUN_REC_PER": "12"}),
    "uniform_compared_stays_crowded_pos4": ("crowded", {**RUNS, **K6, **RECS, **SLOTS}, {"RBG_RUN_REC_PER": "9"}),
    "fillers_super_counts_directories": ("synth", {**RUNS, **K5, **DIRS, **LIST, **POS8, O.OPT_RUN_DEPTHS: 0x1F}, FILL),
    "fillers_super_counts_records": ("synth", {**RUNS, **K5, **RECS, **LIST, **POS8, O.OPT_RUN_DEPTHS: 0x1F}, FILL),
    "automatic": ("synth", RUNS, {}),
}
SWITCHES = ("RBG_RUN_UNIFORM", "RBG_RUN_REC_PER", "RBG_RANK_DIR_RUNS", "RBG_PHI_DIR_PER", "RBG_RUN_FILL_SHIFT", "RBG_PHI_SUPER_SHIFT")


@contextlib.contextmanager
def stderr_of_the_library(lines):
    """what the library (C stdio, file descriptor 2) writes in the block, appended to `lines`"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            yield
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            lines += f.read().decode(errors="replace").splitlines()


def build(arrays, opts, env):
    """one load under the options and switches; the machine-independent fields of rbg_layout_info, two of rbg_info, the verbose lines of the uniform decision"""
    heads, lens, ssa, esa = arrays
    assert not any(k in os.environ for k in SWITCHES + ("RBG_VERBOSE", "RBG_ASSUME_FREE_HBM_MB"))
    os.environ.update({**env, "RBG_VERBOSE": "1", "RBG_ASSUME_FREE_HBM_MB": FREE_MB})
    said = []
    try:
        with contextlib.ExitStack() as st:
            for opt, value in opts.items():
                st.enter_context(capi.default_option(opt, value))
            with stderr_of_the_library(said):
                rb = ra.RowBowt.from_runs(heads, lens, ssa, esa, device=0)
    finally:
        for k in list(env) + ["RBG_VERBOSE", "RBG_ASSUME_FREE_HBM_MB"]:
            del os.environ[k]
    info, li = rb.info(), rb.layout_info()
    rb.close()
    got = {k: int(getattr(li, k)) for k in ("run_fmt", "depths_composed", "depth_mask_asked", "depth_mask_kept", "depths_dropped_budget", "rank_directories",
                                             "phi_directory", "fill_shift", "phi_entries", "phi_fillers", "phi_dir_bytes", "phi_dir_shift", "phi_slots", "phi_slot_bytes")}
    got.update({k: [int(x) for x in getattr(li, k)] for k in ("entries", "fillers", "dir_bytes", "rec_bytes", "rec_overflow")})
    got.update({"layout": int(info.rank_layout), "pos_bytes": int(info.pos_bytes), "hbm_bytes": int(info.hbm_bytes), "info_phi_slots": int(info.phi_slots),
                "uniform_lines": [s.strip() for s in said if "uniform directories" in s]})
    return got


def repeats_index():
    """200 random bases 160 times over: n = 32 001, a few hundred runs -- more than 128 rows per sampled position"""
    import naive
    rng = np.random.default_rng(5)
    text = np.concatenate([np.tile(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 200)], 160), np.array([1], np.uint8)])
    sa = naive.suffix_array(text)
    heads, lens, brk = naive.rle(naive.bwt_from_sa(text, sa))
    ssa, esa = naive.run_samples(sa, brk, len(text))
    assert len(text) >= 128 * len(heads)
    return heads, lens, ssa, esa


def index_of_text(text):
    import naive
    sa = naive.suffix_array(text)
    heads, lens, brk = naive.rle(naive.bwt_from_sa(text, sa))
    ssa, esa = naive.run_samples(sa, brk, len(text))
    return heads, lens, ssa, esa


def random_index():
    """32 000 random bases: nearly every row a run of its own, a 6-mer's table has eight entries on average and many have twelve and more"""
    rng = np.random.default_rng(6)
    return index_of_text(np.concatenate([np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 32000)], np.array([1], np.uint8)]))


def crowded_index():
    """test_gpu_runs.py's crowded text at a twentieth: 400 bases 50 times, then 480 x (one of A,C,G,T + the same 14-mer + 10 random bases)"""
    rng = np.random.default_rng(7)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    block, x = acgt[rng.integers(0, 4, 400)], acgt[rng.integers(0, 4, 14)]
    parts = [block] * 50 + [np.concatenate([acgt[[i % 4]], x, acgt[rng.integers(0, 4, 10)]]) for i in range(480)]
    return index_of_text(np.concatenate(parts + [np.array([1], np.uint8)]))


@pytest.fixture(scope="module")
def indexes(synth):
    return {"synth": (synth.heads, synth.lens, synth.ssa, synth.esa), "repeats": repeats_index(), "random": random_index(), "crowded": crowded_index()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_run_indexed_replica_is_the_recorded_one(indexes, golden, name):
    index, opts, env = CASES[name]
    got = build(indexes[index], opts, env)
    assert got == golden[name], {k: (got[k], golden[name].get(k)) for k in got if got[k] != golden[name].get(k)}


def test_recorded_cases_took_the_branches_they_are_named_for(golden):
    """the golden file itself: each case reached its branch when it was recorded"""
    g = golden
    assert all(g[c]["layout"] == capi.LAYOUT_RUNS and g[c]["run_fmt"] == 2 for c in CASES)
    assert sum(g["directories_pos4"]["dir_bytes"]) > 0 and sum(g["directories_pos4"]["rec_bytes"]) == 0 and g["directories_pos4"]["pos_bytes"] == 4
    assert sum(g["directories_pos8"]["dir_bytes"]) > 0 and g["directories_pos8"]["pos_bytes"] == 8
    assert g["records_pos4"]["rank_directories"] == 0 and sum(g["records_pos4"]["rec_bytes"]) > 0
    assert sum(g["records_pos8_overflowing"]["rec_overflow"]) > 0
    d = g["records_deepest_depth_only"]
    assert [b > 0 for b in d["rec_bytes"][:5]] == [False] * 4 + [True] and d["rank_directories"] == 1 and d["dir_bytes"][0] > 0
    assert g["phi_slots_pos4"]["phi_slots"] > 0 and g["phi_slots_pos4"]["phi_directory"] == 0
    for c, slot_bytes, shift_ok in (("phi_slots_pos4", 16 + 4, True), ("phi_slots_pos8_packed", 16 + 4, True), ("phi_slots_pos8_not_packed", 32 + 4, False)):
        assert g[c]["phi_slot_bytes"] == g[c]["phi_slots"] * slot_bytes and (g[c]["phi_dir_shift"] <= 6) == shift_ok, c
    assert len(g["uniform_forced"]["uniform_lines"]) == 1 and "hot words computed" in g["uniform_forced"]["uniform_lines"][0]
    assert g["uniform_forbidden"]["uniform_lines"] == []
    assert g["uniform_unset"]["uniform_lines"] == g["uniform_forced"]["uniform_lines"] and g["uniform_unset"]["rec_bytes"][7] < g["uniform_forbidden"]["rec_bytes"][7]
    for c in CASES:   # compared: uniform, not forced, and more than one record in 256 overflowing -- or the line that only the comparison prints
        said = " ".join(g[c]["uniform_lines"])
        m = re.search(r"(\d+) of (\d+) overflowing", said)
        compared = "keep their own shifts" in said or (m is not None and c != "uniform_forced" and int(m.group(1)) * 256 > int(m.group(2)))
        assert compared == c.startswith("uniform_compared"), (c, said)
        assert ("keep their own shifts" in said) == ("keep_own_shifts" in c), (c, said)
    for c in ("fillers_super_counts_directories", "fillers_super_counts_records"):
        assert g[c]["fill_shift"] == 5 and all(f > 0 for f in g[c]["fillers"][:5]) and g[c]["phi_fillers"] > 0 and g[c]["phi_directory"] == 1, c
    assert sum(g["fillers_super_counts_directories"]["rec_bytes"]) == 0 and sum(g["fillers_super_counts_records"]["dir_bytes"]) == 0
    a = g["automatic"]
    assert a["depth_mask_kept"] == 0x8B and all(a["rec_bytes"][d] > 0 for d in (0, 1, 3)) and a["phi_slots"] > 0
