#!/usr/bin/env python3
"""Rate of the greedy seed lists (rbg_greedy_seeds_plan_dev + rbg_greedy_seeds_fill_dev, RowBowt::get_seeds_greedy_w_sample
rowbowt.hpp:222-256) and of the toehold checkpoints (rbg_find_range_w_toehold_chkpnts_dev, :575-606) on the bench-shaped index:
100 bp reads with sub_rate 0.1, min_length 10 and 1, wsize 19.  Each is timed with HIP events over --steps steps after --warmup
beside its yardstick on the same reads in the same process: rbg_greedy_longest_seed_dev for the seed lists (the pair walks every
read twice and stores more: about twice its time is the expectation), rbg_find_range_w_toehold_dev for the checkpoints.  One
JSON line per measurement: reads/s, seeds/s, seeds per read, the ratio to the yardstick.  GPU box only."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rowbowt_amd as ra  # noqa: E402
from rowbowt_amd import capi  # noqa: E402
from rowbowt_amd.tools import synth_pangenome as sp  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--L", type=int, default=40_000_000, help="haplotype length of the synthetic pangenome (bench: 40 M)")
ap.add_argument("--H", type=int, default=50, help="haplotypes (bench: 50)")
ap.add_argument("--reads", type=int, default=1_000_000, help="reads per step")
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--min-length", type=int, nargs="+", default=[10, 1])
ap.add_argument("--wsize", type=int, default=19)
args = ap.parse_args()

dev = torch.device("cuda:0")
text, info = sp.make_text(args.L, args.H, 0.01, 20240229, dev)
sa = sp.suffix_array(text)
inp = sp.index_inputs(text, sa)
del sa
m = 100
reads, _ = sp.sample_reads(text, info, args.reads, m, seed=20240231, sub_rate=0.1)
flat = reads.cpu().numpy().reshape(-1)
del text, reads
torch.cuda.empty_cache()
N = args.reads
off = np.arange(N + 1, dtype=np.uint64) * np.uint64(m)
rb = ra.RowBowt.from_runs(inp["heads"], inp["lens"], inp["ssa"], inp["esa"], device=0)
L = ra.lib()
d_seqs = torch.from_numpy(np.concatenate([flat, np.zeros(16, np.uint8)])).to(dev)
d_off = torch.from_numpy(off.view(np.int64)).to(dev)
st = torch.cuda.current_stream().cuda_stream
info_ = rb.info()
print(f"seed lists: n={inp['n']} r={inp['r']} layout={info_.rank_layout} pos_bytes={info_.pos_bytes}, {N} reads x {m} bp, sub_rate 0.1, "
      f"{args.steps} steps after {args.warmup}", flush=True)


def timed(step):
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), min(times), max(times)


def new(n, dtype=torch.int64):
    return torch.empty(max(n, 1), dtype=dtype, device=dev)


one = [new(N) for _ in range(5)]           # the longest-seed call's five arrays / the plain search's three
tmp_bytes = int(L.rbg_greedy_seeds_tmp_bytes(N))
d_tmp = new(tmp_bytes, torch.uint8)
d_soff = new(N + 1)
for ml in args.min_length:
    def longest():
        assert L.rbg_greedy_longest_seed_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, ml, *[t.data_ptr() for t in one], st) == 0
    base_ms, _, _ = timed(longest)
    for flags in (capi.SEEDS_W_SAMPLE, 0):
        box = {"out": None, "ns": 0}

        def pair():
            assert L.rbg_greedy_seeds_plan_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, ml, flags, d_soff.data_ptr(), d_tmp.data_ptr(),
                                               tmp_bytes, st) == 0
            ns = int(d_soff[N].item())         # (the caller sizes its arrays from the plan: the read-back is part of the pair)
            if box["out"] is None or box["out"][0].numel() < ns:
                box["out"] = [new(ns) for _ in range(5)]
            box["ns"] = ns
            assert L.rbg_greedy_seeds_fill_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, ml, flags, d_soff.data_ptr(),
                                               *[t.data_ptr() for t in box["out"]], st) == 0

        def plan_only():
            assert L.rbg_greedy_seeds_plan_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, ml, flags, d_soff.data_ptr(), d_tmp.data_ptr(),
                                               tmp_bytes, st) == 0
        ms, lo, hi = timed(pair)
        plan_ms, _, _ = timed(plan_only)
        ns = box["ns"]
        print(json.dumps({"call": "greedy_seeds_plan+fill", "min_length": ml, "w_sample": bool(flags), "ms_per_step_median": round(ms, 3),
                          "ms_min": round(lo, 3), "ms_max": round(hi, 3), "plan_ms": round(plan_ms, 3), "reads_per_s": N / (ms / 1e3),
                          "seeds_per_s": ns / (ms / 1e3), "seeds_per_read": round(ns / N, 3), "longest_seed_ms": round(base_ms, 3),
                          "ratio_to_longest_seed": round(ms / base_ms, 2)}), flush=True)

# toehold checkpoints beside the plain search with a toehold
w = args.wsize
ctmp = int(L.rbg_toehold_chkpnts_tmp_bytes(N))
d_ctmp = new(ctmp, torch.uint8)
d_slot = new(N + 1)
assert L.rbg_toehold_chkpnts_slots_dev(rb.h, d_off.data_ptr(), N, w, d_slot.data_ptr(), d_ctmp.data_ptr(), ctmp, st) == 0
slots = int(d_slot[N].item())
d_cnt = new(N)
cols = [new(slots) for _ in range(5)]


def plain():
    assert L.rbg_find_range_w_toehold_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, one[0].data_ptr(), one[1].data_ptr(), one[2].data_ptr(), st) == 0


def chk():
    assert L.rbg_toehold_chkpnts_slots_dev(rb.h, d_off.data_ptr(), N, w, d_slot.data_ptr(), d_ctmp.data_ptr(), ctmp, st) == 0
    assert L.rbg_find_range_w_toehold_chkpnts_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, w, d_slot.data_ptr(), d_cnt.data_ptr(),
                                                  *[t.data_ptr() for t in cols], st) == 0


base_ms, _, _ = timed(plain)
ms, lo, hi = timed(chk)
nrec = int(d_cnt[:N].sum().item())
print(json.dumps({"call": "toehold_chkpnts_slots+walk", "wsize": w, "ms_per_step_median": round(ms, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                  "reads_per_s": N / (ms / 1e3), "records_per_s": nrec / (ms / 1e3), "slots": slots, "records": nrec,
                  "reads_that_occur": round(float((d_cnt[:N] > 0).float().mean().item()), 4), "find_range_w_toehold_ms": round(base_ms, 3),
                  "ratio_to_find_range_w_toehold": round(ms / base_ms, 2)}), flush=True)
rb.close()
