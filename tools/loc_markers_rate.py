#!/usr/bin/env python3
"""Rate of the markers at located text positions (rbg_loc_markers_plan_dev + rbg_loc_markers_fill_dev, k_loc_markers.hip) on the
bench-shaped index: 100 bp reads, text markers at a stated density (a run of --run-len positions every --run-every, 1-3 values each).
The locations are uniform random text positions, --per-read of them per read on average (3, 30, 300; the number of reads shrinks so that a
step stays near --locs locations): neighbouring locations of a read come off a phi chain and are unrelated positions, which is what a
uniform draw gives, and the pair sees locations and read lengths only.  Per L / N the pair is timed with HIP events over --steps steps
after --warmup for every forced group width (RBG_LOCMK_GROUP = 4, 16, 64) and unforced, interleaved in ONE process, beside the route a
caller had before: expand every location to a (lo, hi) pair (two torch kernels, 16 bytes per location written and read back) and run
rbg_markers_plan_dev + rbg_markers_fill_dev on the SA-row marker array of the same handle, which holds the same runs -- that gives
per-LOCATION offsets, not per-read ones.  One JSON line per measurement.  GPU box only."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rowbowt_amd as ra  # noqa: E402
from rowbowt_amd.tools import synth_pangenome as sp  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--L", type=int, default=40_000_000, help="haplotype length of the synthetic pangenome (bench: 40 M)")
ap.add_argument("--H", type=int, default=50, help="haplotypes (bench: 50)")
ap.add_argument("--reads", type=int, default=1_000_000, help="reads per step at most")
ap.add_argument("--locs", type=int, default=30_000_000, help="locations per step at most")
ap.add_argument("--per-read", type=int, nargs="+", default=[3, 30, 300])
ap.add_argument("--run-every", type=int, default=1000)
ap.add_argument("--run-len", type=int, default=5)
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

dev = torch.device("cuda:0")
text, info = sp.make_text(args.L, args.H, 0.01, 20240229, dev)
sa = sp.suffix_array(text)
inp = sp.index_inputs(text, sa)
del sa, text
torch.cuda.empty_cache()
n, m = int(inp["n"]), 100
rb = ra.RowBowt.from_runs(inp["heads"], inp["lens"], inp["ssa"], inp["esa"], device=0)
L = ra.lib()
# the same runs in both tables: text positions for the new pair, "SA rows" for the route through rbg_markers_*_dev
starts = np.arange(args.run_every // 2, n - args.run_len - 1, args.run_every, dtype=np.uint64)
ends = starts + np.uint64(args.run_len - 1)
cnt = (np.arange(len(starts)) % 3 + 1).astype(np.uint64)
mk_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
vals = np.arange(int(mk_off[-1]), dtype=np.uint64)
rb.set_text_markers(starts, ends, mk_off, vals)
rb.set_markers(starts, ends, mk_off, vals)
st = torch.cuda.current_stream().cuda_stream
i_ = rb.info()
print(f"loc markers: n={n} r={inp['r']} layout={i_.rank_layout} pos_bytes={i_.pos_bytes}, {len(starts)} runs of {args.run_len} every {args.run_every} "
      f"({int(mk_off[-1])} values), reads of {m} bp, {args.steps} steps after {args.warmup}", flush=True)


def new(k, dtype=torch.int64):
    return torch.empty(max(int(k), 1), dtype=dtype, device=dev)


def one_step(step):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


for per in args.per_read:
    N = max(1, min(args.reads, args.locs // per))
    g = torch.Generator(device=dev)
    g.manual_seed(20240301 + per)
    # per-read counts around `per` (0 .. 2 per), uniform positions
    counts = torch.randint(0, 2 * per + 1, (N,), generator=g, device=dev, dtype=torch.int64)
    d_loc_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    d_loc_off[1:] = torch.cumsum(counts, 0)
    Ltot = int(d_loc_off[N].item())
    d_locs = torch.randint(0, n - m, (max(Ltot, 1),), generator=g, device=dev, dtype=torch.int64)
    d_off = torch.arange(N + 1, dtype=torch.int64, device=dev) * m
    tmp_bytes = int(L.rbg_loc_markers_tmp_bytes(N))
    d_tmp = new(tmp_bytes, torch.uint8)
    d_mk_off = new(N + 1)
    box = {"mk": None, "nmk": 0}

    def pair():
        assert L.rbg_loc_markers_plan_dev(rb.h, d_locs.data_ptr(), d_loc_off.data_ptr(), d_off.data_ptr(), N, d_mk_off.data_ptr(), d_tmp.data_ptr(),
                                          tmp_bytes, st) == 0
        nmk = int(d_mk_off[N].item())          # (the caller sizes its array from the plan: the read-back is part of the pair)
        if box["mk"] is None or box["mk"].numel() < nmk:
            box["mk"] = new(nmk)
        box["nmk"] = nmk
        assert L.rbg_loc_markers_fill_dev(rb.h, d_locs.data_ptr(), d_loc_off.data_ptr(), d_off.data_ptr(), N, d_mk_off.data_ptr(), box["mk"].data_ptr(), st) == 0

    # the route before: expansion + the SA-row pair, per location
    etmp_bytes = int(L.rbg_loc_markers_tmp_bytes(Ltot))
    d_etmp = new(etmp_bytes, torch.uint8)
    d_emk_off = new(Ltot + 1)
    ebox = {"mk": None, "nmk": 0}

    def expanded():
        lo = d_locs[:Ltot]
        hi = lo + (m - 1)                      # (every read is m long here; a ragged batch also needs a gather of the lengths)
        assert L.rbg_markers_plan_dev(rb.h, lo.data_ptr(), hi.data_ptr(), Ltot, d_emk_off.data_ptr(), d_etmp.data_ptr(), etmp_bytes, st) == 0
        nmk = int(d_emk_off[Ltot].item())
        if ebox["mk"] is None or ebox["mk"].numel() < nmk:
            ebox["mk"] = new(nmk)
        ebox["nmk"] = nmk
        assert L.rbg_markers_fill_dev(rb.h, lo.data_ptr(), hi.data_ptr(), Ltot, d_emk_off.data_ptr(), ebox["mk"].data_ptr(), st) == 0

    arms = [("group4", "4"), ("group16", "16"), ("group64", "64"), ("auto", None), ("expanded_route", "x")]
    times = {a[0]: [] for a in arms}
    for rnd in range(args.warmup + args.steps):          # interleaved rounds: every arm once per round
        for name, gval in arms:
            if gval == "x":
                t = one_step(expanded)
            else:
                if gval is None:
                    os.environ.pop("RBG_LOCMK_GROUP", None)
                else:
                    os.environ["RBG_LOCMK_GROUP"] = gval
                t = one_step(pair)
            if rnd >= args.warmup:
                times[name].append(t)
    os.environ.pop("RBG_LOCMK_GROUP", None)
    assert box["nmk"] == ebox["nmk"]
    same = bool((box["mk"][:box["nmk"]] == ebox["mk"][:ebox["nmk"]]).all().item())     # (equal-length reads: the two orders coincide)
    base = float(np.median(times["expanded_route"]))
    for name, _g in arms:
        ms = float(np.median(times[name]))
        print(json.dumps({"call": "loc_markers_plan+fill" if name != "expanded_route" else "expand + markers_plan+fill", "arm": name, "per_read": per,
                          "reads": N, "locations": Ltot, "locations_per_read": round(Ltot / N, 2), "markers": box["nmk"],
                          "markers_per_location": round(box["nmk"] / max(Ltot, 1), 3), "ms_median": round(ms, 3), "ms_min": round(min(times[name]), 3),
                          "ms_max": round(max(times[name]), 3), "locations_per_s": Ltot / (ms / 1e3), "ratio_to_expanded_route": round(ms / base, 3),
                          "same_values_as_expanded_route": same}), flush=True)
rb.close()
