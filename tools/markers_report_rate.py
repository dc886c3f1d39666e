#!/usr/bin/env python3
"""Milliseconds per step of rb_markers' report on the device (include/rbg.h: rbg_markers_report_text and its device steps) on the bench-shaped
index with its synthetic marker array: 100 bp reads with sub_rate 0.1, wsize 19, max_range 1000.  The device steps -- strands
(rbg_read_strands_dev), plan + fill of the seeds with the log (rbg_marker_seeds_plan_log_dev / _fill_log_dev), canon
(rbg_marker_seeds_canon_dev), select (rbg_report_select_dev) -- are timed one by one with HIP events over --steps steps after --warmup, in
the default mode and in `--heuristic --best-strand-only --min-seed-length 30`.  The text kernels have no entry point of their own: the
whole host call (rbg_markers_report_text: copy in, the steps above, the text, copy out) is timed by the wall clock, and run once more with
RBG_REPORT_TRACE=1 in a child process, whose per-step sums (each step synchronised) go to stderr.  One JSON line per measurement.  GPU box only."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

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
ap.add_argument("--reads", type=int, default=262_144, help="reads per step (rb_markers' batch)")
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--wsize", type=int, default=19)
ap.add_argument("--max-range", type=int, default=1000)
ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()

dev = torch.device("cuda:0")
text, info = sp.make_text(args.L, args.H, 0.01, 20240229, dev)
sa = sp.suffix_array(text)
inp = sp.index_inputs(text, sa)
markers = sp.marker_array(text, info, sa, w=10)
del sa
m = 100
reads, _ = sp.sample_reads(text, info, args.reads, m, seed=20240231, sub_rate=0.1)
flat = reads.cpu().numpy().reshape(-1)
del text, reads
torch.cuda.empty_cache()
N = args.reads
off = np.arange(N + 1, dtype=np.uint64) * np.uint64(m)
rb = ra.RowBowt.from_runs(inp["heads"], inp["lens"], inp["ssa"], inp["esa"], device=0)
rb.set_markers(*markers)
L = ra.lib()
names = [b"read%d" % i for i in range(N)]
MODES = {"default": capi.report_params(wsize=args.wsize, max_range=args.max_range),
         "heuristic-best-strand-y30": capi.report_params(wsize=args.wsize, max_range=args.max_range, heuristic=True, best_strand=True, min_seed_len=30)}
coins = (np.arange(N) % 2).astype(np.uint8)


def host_call(params):
    t0 = time.perf_counter()
    out = rb.markers_report_text(flat, off, names, params, coins)
    return (time.perf_counter() - t0) * 1e3, len(out)


if args.traced_child:   # (RBG_REPORT_TRACE is read when the library loads: the sums are printed at exit)
    for params in MODES.values():
        for _ in range(args.warmup + args.steps):
            host_call(params)
    sys.exit(0)

print(f"markers report: n={inp['n']} r={inp['r']} {len(markers[0])} marker runs, {N} reads x {m} bp, wsize {args.wsize}, max_range {args.max_range}, "
      f"{args.steps} steps after {args.warmup}", flush=True)
st = torch.cuda.current_stream().cuda_stream


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


def ok(rc):
    assert rc == 0, rc


d_raw = torch.from_numpy(np.concatenate([flat, np.zeros(16, np.uint8)])).to(dev)
d_off = torch.from_numpy(off.view(np.int64)).to(dev)
total = N * m
d_seq2 = new(L.rbg_read_strands_bytes(total), torch.uint8)
d_off2 = new(2 * N + 1)
N2 = 2 * N
d_soff, d_moff = new(N2 + 1), new(N2 + 1)
tmp_bytes = L.rbg_locate_plan_tmp_bytes(N2)
d_tmp = new(tmp_bytes, torch.uint8)
log_bytes = L.rbg_marker_seeds_log_bytes(rb.h, N2, 0)
d_log = new(log_bytes, torch.uint8)


def strands():
    ok(L.rbg_read_strands_dev(rb.h, d_raw.data_ptr(), d_off.data_ptr(), N, total, d_seq2.data_ptr(), d_off2.data_ptr(), st))


def plan():
    ok(L.rbg_marker_seeds_plan_log_dev(rb.h, d_seq2.data_ptr(), d_off2.data_ptr(), N2, args.wsize, args.max_range, 0, d_soff.data_ptr(), d_moff.data_ptr(),
                                       d_tmp.data_ptr(), tmp_bytes, d_log.data_ptr(), log_bytes, st))


rows = {"strands": timed(strands), "plan": timed(plan)}
S, M = int(d_soff[-1].item()), int(d_moff[-1].item())
d_seeds, d_mk = new(6 * S), new(M)
ctmp_bytes = L.rbg_marker_seeds_canon_tmp_bytes(S)
d_ctmp = new(ctmp_bytes, torch.uint8)
d_rep, d_recs, d_read = new(N + 1), new(6 * S), new(S, torch.int32)
stmp_bytes = L.rbg_report_select_tmp_bytes(N)
d_stmp = new(stmp_bytes, torch.uint8)
d_coin = torch.from_numpy(coins).to(dev)


def fill():
    plan()   # (the fill consumes the plan's log)
    ok(L.rbg_marker_seeds_fill_log_dev(rb.h, d_seq2.data_ptr(), d_off2.data_ptr(), N2, args.wsize, args.max_range, 0, d_soff.data_ptr(), d_moff.data_ptr(),
                                       d_seeds.data_ptr(), d_mk.data_ptr(), d_log.data_ptr(), log_bytes, st))


rows["plan+fill"] = timed(fill)
for mode, params in MODES.items():
    cflags = params.flags & (capi.REPORT_CLEAR_CONFLICTING | capi.REPORT_CLEAR_IDENTICAL)

    def canon():
        fill()   # (canon works in place: every step starts from fresh records)
        ok(L.rbg_marker_seeds_canon_dev(rb.h, d_seeds.data_ptr(), S, d_mk.data_ptr(), params.min_range, cflags, params.read_len, d_ctmp.data_ptr(), ctmp_bytes, st))

    def select():
        ok(L.rbg_report_select_dev(rb.h, d_seeds.data_ptr(), d_soff.data_ptr(), d_off2.data_ptr(), N, d_coin.data_ptr(), C.byref(params), d_rep.data_ptr(),
                                   d_recs.data_ptr(), d_read.data_ptr(), d_stmp.data_ptr(), stmp_bytes, st))

    rows[f"{mode}: plan+fill+canon"] = timed(canon)
    rows[f"{mode}: select"] = timed(select)
    for _ in range(args.warmup):
        host_call(params)
    calls = [host_call(params) for _ in range(args.steps)]
    ms = [c[0] for c in calls]
    rows[f"{mode}: whole host call"] = (float(np.median(ms)), min(ms), max(ms))
    print(json.dumps({"mode": mode, "text_bytes_per_read": calls[0][1] / N, "printed_records": int(d_rep[-1].item()), "seed_records": S, "markers": M}), flush=True)
for what, (med, lo, hi) in rows.items():
    print(json.dumps({"step": what, "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reads": N, "reads_per_s": N / (med * 1e-3)}), flush=True)
p = subprocess.run([sys.executable, os.path.abspath(__file__), "--traced-child"] + [a for a in sys.argv[1:]], env=dict(os.environ, RBG_REPORT_TRACE="1"),
                   capture_output=True, text=True)
print("\n".join(line for line in p.stderr.splitlines() if line.startswith("rbg_markers_report")), flush=True)
