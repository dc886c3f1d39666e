#!/usr/bin/env python3
"""Rate of the lmem marker seeds (rbg_marker_lmems_plan_dev + rbg_marker_lmems_fill_dev, RowBowt::get_markers_lmems
rowbowt.hpp:341-404) on the bench-shaped index with its synthetic marker array: 100 bp reads on both strands, wsize 19,
max_range 1000, ftab_k 0 and 12.  The device pair is timed with HIP events over --steps steps after --warmup; the printed line
gives reads/s (a read = both strands), end positions/s, ms per step and the bytes written.  GPU box only."""
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
ap.add_argument("--reads", type=int, default=100_000, help="reads per step (2 strands each)")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--ftab-k", type=int, nargs="+", default=[0, 12])
args = ap.parse_args()

dev = torch.device("cuda:0")
text, info = sp.make_text(args.L, args.H, 0.01, 20240229, dev)
sa = sp.suffix_array(text)
inp = sp.index_inputs(text, sa)
markers = sp.marker_array(text, info, sa, w=10)
del sa
m = 100
reads, _ = sp.sample_reads(text, info, args.reads, m, seed=20240231, sub_rate=0.1)
fwd = reads.cpu().numpy()
del text, reads
torch.cuda.empty_cache()
comp = np.zeros(256, np.uint8)
for a, b in zip(b"ACGT", b"TGCA"):
    comp[a] = b
strands = np.empty((2 * args.reads, m), np.uint8)
strands[0::2] = fwd
strands[1::2] = comp[fwd[:, ::-1]]
N = 2 * args.reads
total = N * m
off = np.arange(N + 1, dtype=np.uint64) * np.uint64(m)
rb = ra.RowBowt.from_runs(inp["heads"], inp["lens"], inp["ssa"], inp["esa"], device=0)
rb.set_markers(*markers)
L = ra.lib()
d_seqs = torch.from_numpy(np.concatenate([strands.reshape(-1), np.zeros(16, np.uint8)])).to(dev)
d_off = torch.from_numpy(off.view(np.int64)).to(dev)
tmp_bytes = int(L.rbg_marker_lmems_tmp_bytes(N, total))
d_tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=dev)
d_moff = torch.empty(N + 1, dtype=torch.int64, device=dev)
d_rec = torch.empty(6 * total, dtype=torch.int64, device=dev)
st = torch.cuda.current_stream().cuda_stream
info_ = rb.info()
print(f"lmem marker seeds: n={inp['n']} r={inp['r']} layout={info_.rank_layout} pos_bytes={info_.pos_bytes}, {args.reads} reads x 2 strands x {m} bp, "
      f"wsize 19, max_range 1000, {args.steps} steps after {args.warmup}", flush=True)
for K in args.ftab_k:
    def step():
        assert L.rbg_marker_lmems_plan_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, total, 19, 1000, K, d_moff.data_ptr(),
                                           d_tmp.data_ptr(), tmp_bytes, st) == 0
        nmk = int(d_moff[-1].item())
        if step.mk is None or step.mk.numel() < max(nmk, 1):
            step.mk = torch.empty(max(nmk, 1), dtype=torch.int64, device=dev)
        assert L.rbg_marker_lmems_fill_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, total, 19, 1000, K, d_tmp.data_ptr(),
                                           d_rec.data_ptr(), step.mk.data_ptr(), st) == 0
        return nmk
    step.mk = None
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        nmk = step()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    ms = float(np.median(times))
    rec = d_rec[:6 * total].view(total, 6).cpu().numpy().view(np.uint64)
    mean_len = float((rec[:, 3] - rec[:, 2]).mean())
    out = {"ftab_k": K, "ms_per_step_median": round(ms, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
           "reads_per_s": args.reads / (ms / 1e3), "end_positions_per_s": total / (ms / 1e3),
           "bytes_written": total * 48 + nmk * 8 + (N + 1) * 8, "records": total, "markers": nmk, "mean_seed_len": round(mean_len, 2)}
    print(json.dumps(out), flush=True)
rb.close()
