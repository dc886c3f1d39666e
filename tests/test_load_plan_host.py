"""CPU check of the load rules (rbg_load_plan.hpp: budget and its raise, planned depth, slot levels, the run-indexed layout's depth trimming and bucket
records, widen shift, ftab, jump budgets; the geometry of the run-indexed layout: bucket shifts, the uniform depth's candidate and verdict, phi slots and
phi directory, the read-staging tables) as functions of plain numbers -- the rules that otherwise fire only at r = 1e9 on a whole device, or only with a GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import layout_rules_table  # noqa: E402


def test_load_rules_by_hand_and_against_the_recorded_loads(tmp_path):
    """tests/cpp/load_plan_check.cpp under ASan + UBSan.  Expectations worked out by hand from the rules as stated (thresholds from both sides: the budget's
    `>`, nine tenths of the device, the 40-bit ranks of wide slots, 4e9 ftab words, half of the free memory, half of the replica); and the four committed
    default loads (tools/layout_rules_table.py DEFAULT): budget, raise and planned depth must be what those loads recorded.  The geometry rules: every
threshold from both sides (the bucket shift's <=, 1.1 x the own records, the 27-bit stride, one record in 256, a quarter more overflow, 2 r phi buckets,
the packed slots' three conditions), and the stage tables of ACGT, acgt and 20 000 random byte subsets against a brute-force search of the shift."""
    rows = []
    for path in layout_rules_table.DEFAULT:
        ix = layout_rules_table.load(path)["config"]["index"]
        li = ix.get("layout_info") or {}
        rows += [ix["n"], ix["r"], ix["hbm_free_at_load"], ix["hbm_budget"], li.get("budget_raised", 0), ix["symbols_per_gather"]]
    assert len(rows) == 24
    exe = tmp_path / "load_plan"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "load_plan_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)] + [str(int(x)) for x in rows], capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith(b"load_plan ok rows 4 checks "), p.stdout[-2000:] + p.stderr[-600:]
