#!/usr/bin/env python3
"""Milliseconds of the marker tally (include/rbg.h: rbg_markers_tally, rbg_tally_add_dev) on the bench-shaped index with its synthetic marker
array: 100 bp reads with sub_rate 0.1, wsize 19, max_range 1000, rb_markers' default mode.  Everything is timed with HIP events in this one
process, over --steps steps after --warmup, for the reads in random order and sorted by coordinate (where neighbours share markers):
  - the device steps one by one -- strands, plan, plan + fill, plan + fill + canon, select, as tools/markers_report_rate.py times them -- and the
    add (rbg_tally_add_dev on select's records) into an empty table and into one that holds the keys already, with the combining of equal keys
    within a wave on and off (RBG_TALLY_COMBINE);
  - the whole host calls on the same reads: rbg_markers_report (records), rbg_markers_report_text and rbg_markers_tally (combining on and off;
    one tally fed by every step, so its reserve rule and its grows are part of the time);
  - the per-read mode beside the line mode: the add (rbg_tally_add_reads_dev with RBG_TALLY_PER_READ and with | RBG_TALLY_DROP_SITE_CONFLICTS) next
    to rbg_tally_add_dev, and the three whole calls (rbg_markers_tally; rbg_markers_tally_reads per read; per read + site rule) on the same reads,
    three runs each after one warm-up, each into a tally of its own that holds the keys after the warm-up.  The verdict lines compare the SLOWEST
    of a per-read mode's three with the FASTEST of the line mode's three.
One JSON line per measurement.  GPU box only."""
import argparse
import ctypes as C
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
ap.add_argument("--reads", type=int, default=262_144, help="reads per step (rb_markers' batch)")
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--wsize", type=int, default=19)
ap.add_argument("--max-range", type=int, default=1000)
args = ap.parse_args()

dev = torch.device("cuda:0")
text, info = sp.make_text(args.L, args.H, 0.01, 20240229, dev)
sa = sp.suffix_array(text)
inp = sp.index_inputs(text, sa)
markers = sp.marker_array(text, info, sa, w=10)
del sa
m = 100
reads, start = sp.sample_reads(text, info, args.reads, m, seed=20240231, sub_rate=0.1)
by_coord = torch.argsort(start % info["unit"])            # the same locus of every haplotype side by side
ORDERS = {"random": reads.cpu().numpy().reshape(-1), "sorted": reads[by_coord].cpu().numpy().reshape(-1)}
del text, reads, start, by_coord
torch.cuda.empty_cache()
N = args.reads
off = np.arange(N + 1, dtype=np.uint64) * np.uint64(m)
rb = ra.RowBowt.from_runs(inp["heads"], inp["lens"], inp["ssa"], inp["esa"], device=0)
rb.set_markers(*markers)
L = ra.lib()
names = [b"read%d" % i for i in range(N)]
params = capi.report_params(wsize=args.wsize, max_range=args.max_range)
print(f"marker tally: n={inp['n']} r={inp['r']} {len(markers[0])} marker runs, {N} reads x {m} bp, wsize {args.wsize}, max_range {args.max_range}, "
      f"{args.steps} steps after {args.warmup}", flush=True)
st = torch.cuda.current_stream().cuda_stream
MODES = (("line", 0), ("per read", capi.TALLY_PER_READ), ("per read + site rule", capi.TALLY_PER_READ | capi.TALLY_DROP_SITE_CONFLICTS))


def timed(step, before=None):
    times = []
    for i in range(args.warmup + args.steps):
        if before:
            before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        if i >= args.warmup:
            times.append(a.elapsed_time(b))
    return float(np.median(times)), min(times), max(times)


def new(n, dtype=torch.int64):
    return torch.empty(max(n, 1), dtype=dtype, device=dev)


def ok(rc):
    assert rc == 0, rc


def combine(on):
    os.environ["RBG_TALLY_COMBINE"] = "1" if on else "0"   # (read by the library at every launch)


total = N * m
N2 = 2 * N
for order, flat in ORDERS.items():
    rows = {}
    d_raw = torch.from_numpy(np.concatenate([flat, np.zeros(16, np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_seq2 = new(L.rbg_read_strands_bytes(total), torch.uint8)
    d_off2 = new(N2 + 1)
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

    rows["strands"] = timed(strands)
    rows["plan"] = timed(plan)
    S, M_raw = int(d_soff[-1].item()), int(d_moff[-1].item())
    d_seeds, d_mk = new(6 * S), new(M_raw)
    ctmp_bytes = L.rbg_marker_seeds_canon_tmp_bytes(S)
    d_ctmp = new(ctmp_bytes, torch.uint8)
    d_rep, d_recs, d_read = new(N + 1), new(6 * S), new(S, torch.int32)
    stmp_bytes = L.rbg_report_select_tmp_bytes(N)
    d_stmp = new(stmp_bytes, torch.uint8)

    def fill():
        plan()   # (the fill consumes the plan's log)
        ok(L.rbg_marker_seeds_fill_log_dev(rb.h, d_seq2.data_ptr(), d_off2.data_ptr(), N2, args.wsize, args.max_range, 0, d_soff.data_ptr(), d_moff.data_ptr(),
                                           d_seeds.data_ptr(), d_mk.data_ptr(), d_log.data_ptr(), log_bytes, st))

    def canon():
        fill()   # (canon works in place: every step starts from fresh records)
        ok(L.rbg_marker_seeds_canon_dev(rb.h, d_seeds.data_ptr(), S, d_mk.data_ptr(), params.min_range, 0, params.read_len, d_ctmp.data_ptr(), ctmp_bytes, st))

    def select():
        ok(L.rbg_report_select_dev(rb.h, d_seeds.data_ptr(), d_soff.data_ptr(), d_off2.data_ptr(), N, None, C.byref(params), d_rep.data_ptr(),
                                   d_recs.data_ptr(), d_read.data_ptr(), d_stmp.data_ptr(), stmp_bytes, st))

    rows["plan+fill"] = timed(fill)
    rows["plan+fill+canon"] = timed(canon)
    rows["select"] = timed(select)
    R = int(d_rep[-1].item())
    atmp_bytes = L.rbg_tally_add_tmp_bytes(R)
    d_atmp = new(atmp_bytes, torch.uint8)
    t = capi.Tally(rb, M_raw)   # (room for every element of a step as a key of its own: no grow inside the timed add)

    def add():
        ok(L.rbg_tally_add_dev(t.h, d_recs.data_ptr(), R, d_mk.data_ptr(), M_raw, d_atmp.data_ptr(), atmp_bytes, st))

    def empty():
        t.reset()
        t.reserve(M_raw)

    def full():
        t.reserve(M_raw)   # (the bound has grown by a step's elements: an exact read, no grow)

    for on in (True, False):
        combine(on)
        tag = "combining on" if on else "combining off"
        rows[f"add into an empty table, {tag}"] = timed(add, empty)
        rows[f"add, keys present, {tag}"] = timed(add, full)
    rtmp_bytes = L.rbg_tally_add_reads_tmp_bytes(N, R)
    d_rtmp = new(rtmp_bytes, torch.uint8)
    combine(True)
    for tag, flags in MODES[1:]:
        def add_reads():
            ok(L.rbg_tally_add_reads_dev(t.h, d_recs.data_ptr(), R, d_rep.data_ptr(), N, d_mk.data_ptr(), M_raw, flags, d_rtmp.data_ptr(), rtmp_bytes, st))

        rows[f"add {tag}, into an empty table"] = timed(add_reads, empty)
        rows[f"add {tag}, keys present"] = timed(add_reads, full)
        ri = t.read_info()
        print(json.dumps({"order": order, "mode": tag, "read_info after the adds": ri}), flush=True)
    del d_rtmp
    empty()
    add()
    i = t.info()   # (synchronises)
    print(json.dumps({"order": order, "printed_records": R, "seed_records": S, "elements_upper_bound": M_raw, "elements": i["elements"],
                      "distinct_markers": i["entries"], "capacity": i["capacity"], "dropped": i["dropped"]}), flush=True)
    t.close()
    del d_seeds, d_mk, d_recs, d_read, d_log, d_seq2

    def call_report():
        rb.markers_report(flat, off, params, None)

    def call_text():
        rb.markers_report_text(flat, off, names, params, None)

    rows["whole call: rbg_markers_report"] = timed(call_report)
    rows["whole call: rbg_markers_report_text"] = timed(call_text)
    for on in (True, False):
        combine(on)
        t = capi.Tally(rb, 0)   # (the default handle: its grows are inside the warm-up or the time, as they fall)

        def call_tally():
            rb.markers_tally(flat, off, params, None, t)

        rows[f"whole call: rbg_markers_tally, {'combining on' if on else 'combining off'}"] = timed(call_tally)
        i = t.info()
        print(json.dumps({"order": order, "tally after the calls": i}), flush=True)
        t.close()
    combine(True)
    three = {}
    for tag, flags in MODES:   # the same reads, three runs each after one warm-up
        t = capi.Tally(rb, 0)

        def call_mode():
            rb.markers_tally(flat, off, params, None, t, flags=flags)

        call_mode()
        ms = []
        for _ in range(3):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call_mode()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        three[tag] = ms
        print(json.dumps({"order": order, "whole call, three runs": tag, "ms": [round(x, 4) for x in ms], "info": t.info(), "read_info": t.read_info()}), flush=True)
        t.close()
    for tag, _ in MODES[1:]:
        print(json.dumps({"order": order, "mode": tag, "slowest of three / fastest of three of the line mode": round(max(three[tag]) / min(three["line"]), 4)}),
              flush=True)
    for what, (med, lo, hi) in rows.items():
        print(json.dumps({"order": order, "step": what, "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reads": N,
                          "reads_per_s": N / (med * 1e-3)}), flush=True)
    verdict = rows["whole call: rbg_markers_tally, combining on"][2] <= rows["whole call: rbg_markers_report"][1]
    print(json.dumps({"order": order, "tally slowest <= report fastest (this run)": bool(verdict)}), flush=True)
rb.close()
