"""bench.py's command line: a plain run times the headline only (the other legs need --full), --steps sets the number of
timed steps, and --dump-outputs writes what the last timed step computed, the same for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--L", "1500000", "--H", "8", "--reads", "150000"]


def clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}


@pytest.mark.parametrize("leg", [["--markers"], ["--two-stream"], ["--replicas", "2"]])
def test_legs_beside_the_headline_need_full(leg):
    """refused before torch is imported or a device is touched"""
    p = subprocess.run([sys.executable, BENCH, *leg], capture_output=True, text=True, timeout=120, env=clean_env())
    assert p.returncode != 0 and "--full" in p.stderr and leg[0] in p.stderr and p.stdout.strip() == ""


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120, env=clean_env())
    assert p.returncode != 0 and "--steps" in p.stderr and p.stdout.strip() == ""


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    """Two plain runs with different --steps: each line holds the headline fields and none of --full's blocks, its counters
    count exactly the timed steps, and both dumps are the same float64 arrays, consistent with each other."""
    dumps = []
    for steps in (2, 3):
        d = tmp_path / f"s{steps}"
        p = subprocess.run([sys.executable, BENCH, "--steps", str(steps), "--warmup", "1", *SMALL, "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT, env=clean_env())
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["steps"] == steps and line["warmup"] == 1 and line["full"] is False
        assert line["higher_is_better"] is True and line["unit"] == "reads/s" and line["metric"].startswith("reads/s (100 bp")
        assert line["ms_per_step"] > 0 and abs(line["value"] - 150000 * 1e3 / line["ms_per_step"]) <= 1e-6 * line["value"]
        assert line["counters"]["reads"] == 150000 * steps and line["counters"]["sum_occ"] == line["counters"]["sum_locs"]
        assert not {"parity", "properties_full_size", "count_only", "markers", "kernels", "roofline", "space_speed", "cpu_baseline"} & set(line)
        arrays = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
        assert set(arrays) == {"read_index", "lo", "hi", "toehold", "loc_off", "occ", "locs", "batch_sums"}
        assert all(a.dtype == np.float64 for a in arrays.values()) and sum(a.nbytes for a in arrays.values()) < 64 << 20
        dumps.append((arrays, line["counters"]["sum_locs"] // steps))
    (a, locs_per_step), (b, _) = dumps
    assert all(np.array_equal(a[k], b[k]) for k in a)
    matched = a["hi"] >= a["lo"]
    assert (a["occ"] == np.where(matched, a["hi"] - a["lo"] + 1, 0)).all() and matched.any()
    assert len(a["locs"]) == a["occ"].sum() and a["batch_sums"][-1] == locs_per_step
