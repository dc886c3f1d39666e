#!/usr/bin/env python3
"""Rates of the extract calls (include/rbg.h: rbg_extract_prepare, rbg_isa_dev, rbg_extract_dev, rbg_extract) on the bench-shaped index with hap<h> documents:

    prepare         rbg_extract_prepare's time and the ISA sample's bytes (rbg_fl_prepare first, timed apart)
    rbg_isa_dev     positions/s on --positions random positions
    rbg_extract_dev bases/s for --items items of 100 bp at random positions, packed output
    rbg_extract     one whole document from host memory, for every RBG_OPT_EXTRACT_CHUNK of --chunks

Each device call is timed on the host from its start to its return (the calls wait for their stream; inputs and outputs live on the device), the median of
--steps after --warmup, with the range.  THE YARDSTICK stands beside each rate: the same count of FL steps -- the walk-ins, counted here from the run-end
samples, plus the bases -- through rbg_fl_dev over random rows, --positions rows a call, in the same process, ALTERNATING with the measured call.  One JSON line per measurement.  GPU box only; no test runs this."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--L", type=int, default=40_000_000, help="haplotype length of the synthetic pangenome (bench: 40 M)")
ap.add_argument("--H", type=int, default=50, help="haplotypes = documents (bench: 50)")
ap.add_argument("--positions", type=int, default=10_000_000)
ap.add_argument("--items", type=int, default=1_000_000)
ap.add_argument("--chunks", type=int, nargs="*", default=[64, 128, 256, 512, 1024, 4096])
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rowbowt_amd as ra  # noqa: E402
from rowbowt_amd import capi  # noqa: E402
from rowbowt_amd.tools import synth_pangenome as sp  # noqa: E402

dev = torch.device("cuda:0")
text, info = sp.make_text(args.L, args.H, 0.01, 20240229, dev)
sa = sp.suffix_array(text)
inp = sp.index_inputs(text, sa)
del sa, text
torch.cuda.empty_cache()
n, H = int(inp["n"]), info["H"]
rb = ra.RowBowt.from_runs(inp["heads"], inp["lens"], inp["ssa"], inp["esa"], device=0)
rb.set_docs([f"hap{h}" for h in range(H)], [h * info["unit"] for h in range(H)])
L = ra.lib()
print(f"extract rate: n={n} r={inp['r']} {H} documents, {args.steps} steps after {args.warmup}", flush=True)

t0 = time.perf_counter()
rb.fl_prepare()
fl_ms = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
rb.extract_prepare()
ex_ms = (time.perf_counter() - t0) * 1e3
print(json.dumps({"what": "rbg_fl_prepare", "ms": fl_ms, **rb.fl_info()}), flush=True)
print(json.dumps({"what": "rbg_extract_prepare (FL index already there)", "ms": ex_ms, **rb.extract_info()}), flush=True)

# the samples' text positions (every run's last row; the synthetic text has no byte that is no base but its terminator): the walk-in of p is p - the sample before
tpos = np.sort(np.asarray(inp["esa"], dtype=np.uint64))
assert int(tpos[0]) == 0 and len(tpos) == rb.extract_info()["samples"]
rng = np.random.default_rng(20240301)
st = lambda: torch.cuda.current_stream().cuda_stream
up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(dev)


def walk_in(pos):
    return int((pos - tpos[np.searchsorted(tpos, pos, side="right") - 1]).sum())


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


d_rows = up(rng.integers(0, n, args.positions).astype(np.uint64), np.int64)
d_sym = torch.empty(args.positions, dtype=torch.uint8, device=dev)
d_next = torch.empty(args.positions, dtype=torch.int64, device=dev)


def fl_steps(count):
    """`count` FL steps through rbg_fl_dev: whole calls of --positions rows, the last one shorter"""
    left = count
    while left > 0:
        m = min(left, args.positions)
        assert L.rbg_fl_dev(rb.h, d_rows.data_ptr(), m, d_sym.data_ptr(), d_next.data_ptr(), st()) == 0
        left -= m


def pair(what, fn, steps, unit, count, extra=None):
    a, y = [], []
    for i in range(args.warmup + args.steps):              # the two alternate, call by call
        ta, ty = clock(fn), clock(lambda: fl_steps(steps))
        if i >= args.warmup:
            a.append(ta)
            y.append(ty)
    med, ymed = float(np.median(a)), float(np.median(y))
    print(json.dumps({"what": what, **(extra or {}), "ms_median": med, "ms_min": min(a), "ms_max": max(a), unit + "_per_s": count / (med / 1e3), "fl_steps": steps,
                      "fl_steps_per_s": steps / (med / 1e3), "yardstick": "rbg_fl_dev, the same count of FL steps", "yardstick_ms_median": ymed,
                      "yardstick_ms_min": min(y), "yardstick_ms_max": max(y), "yardstick_fl_steps_per_s": steps / (ymed / 1e3)}), flush=True)


# rbg_isa_dev
pos = rng.integers(0, n, args.positions).astype(np.uint64)
d_pos, d_row = up(pos, np.int64), torch.empty(args.positions, dtype=torch.int64, device=dev)
pair("rbg_isa_dev", lambda: L.rbg_isa_dev(rb.h, d_pos.data_ptr(), args.positions, d_row.data_ptr(), st()), walk_in(pos), "positions", args.positions,
     {"positions": args.positions})

# rbg_extract_dev: items of 100 bp inside the documents
m = 100
doc = rng.integers(0, H, args.items).astype(np.uint64)
ipos = doc * np.uint64(info["unit"]) + rng.integers(0, args.L - m, args.items).astype(np.uint64)
d_ipos, d_len = up(ipos, np.int64), torch.full((args.items,), m, dtype=torch.int32, device=dev)
d_off = up(np.arange(args.items, dtype=np.uint64) * np.uint64(m), np.int64)
d_out, d_got = torch.empty(args.items * m, dtype=torch.uint8, device=dev), torch.empty(args.items, dtype=torch.int32, device=dev)
pair("rbg_extract_dev", lambda: L.rbg_extract_dev(rb.h, d_ipos.data_ptr(), d_len.data_ptr(), d_off.data_ptr(), args.items, d_out.data_ptr(), d_got.data_ptr(), st()),
     walk_in(ipos) + args.items * m, "bases", args.items * m, {"items": args.items, "len": m})
assert int(d_got.sum().item()) == args.items * m

# rbg_extract: the whole of one document from host memory, per chunk (the walk-ins are those of the pieces' first positions)
dstart, dlen = np.array([(H // 2) * info["unit"]], np.uint64), np.array([args.L], np.uint64)
out, got = np.zeros(args.L, np.uint8), np.zeros(1, np.uint64)
first = None
for chunk in args.chunks:
    capi.set_default_option(capi.OPT_EXTRACT_CHUNK, chunk)
    pp = dstart[0] + np.arange(0, args.L, chunk, dtype=np.uint64)
    pair("rbg_extract, one document from host memory", lambda: capi._check(L.rbg_extract(rb.h, capi._p(dstart), capi._p(dlen), 1, capi._p(out), capi._p(got)), "rbg_extract"),
         walk_in(pp) + args.L, "bases", args.L, {"chunk": chunk, "bases": args.L, "pieces": len(pp)})
    assert int(got[0]) == args.L
    first = out.copy() if first is None else first
    assert (out == first).all()                             # the result does not depend on the chunk
capi.set_default_option(capi.OPT_EXTRACT_CHUNK, 128)
rb.close()
