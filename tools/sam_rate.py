#!/usr/bin/env python3
"""Milliseconds of rbg_align_sam (include/rbg.h) on the bench-shaped index with hap<h> documents attached: --reads reads of 100 bp, half of them
reverse-complemented, at sub_rate 0 and 0.1, with RBG_SAM_SECONDARY off and on (max_hits 16, min_length 20), qualities present.  Every call is
timed on the host from its start to the end of rbg_wait_text (inputs in pageable host memory, prepacked: no Python work inside the clock), the
median of --steps after --warmup.  For context the same reads go through rbg_find_range_w_toehold + rbg_align_text (one strand, every location on one
line: another output, the same machinery), and through rbg_align_sam_extend (the same lines with every seed extended leftwards by an LF walk, --max-mismatch,
default 4: the yardstick of that row is the rbg_align_sam row beside it); and through rbg_align_sam_extend_both (the right clip extended too, by an FL walk; its yardstick is the rbg_align_sam_extend row); the calls ALTERNATE call by call in one process, since calls later in a process are
slower whatever they run.
--trace: one configuration (--sub-rate, --secondary; --extend: the extended call) with RBG_SAM_TRACE=1, every step of the call synchronised: the library prints
the split copy in / strands / search / pick / locate / [extend /] text plan / text fill / copy out at exit (those calls are slower than untraced ones: the
steps no longer overlap), and for the extended call the sums of its lines' records: lines, lines with a clipped prefix, LF steps, mismatches taken (every
other step hit at its first request), lines extended and by how many bases, left clips gone.
One JSON line per measurement.  GPU box only."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--L", type=int, default=40_000_000, help="haplotype length of the synthetic pangenome (bench: 40 M)")
ap.add_argument("--H", type=int, default=50, help="haplotypes = documents (bench: 50)")
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--trace", action="store_true", help="one configuration with RBG_SAM_TRACE=1 (the split of the call)")
ap.add_argument("--sub-rate", type=float, default=0.1, help="--trace: the configuration's sub_rate")
ap.add_argument("--secondary", action="store_true", help="--trace: with RBG_SAM_SECONDARY")
ap.add_argument("--extend", action="store_true", help="--trace: rbg_align_sam_extend instead of rbg_align_sam")
ap.add_argument("--both", action="store_true", help="--trace: rbg_align_sam_extend_both (the right clip extended too, by an FL walk)")
ap.add_argument("--max-mismatch", type=int, default=4, help="the budget of rbg_align_sam_extend")
args = ap.parse_args()
if args.trace:
    os.environ["RBG_SAM_TRACE"] = "1"   # (read when the library is loaded)

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
del sa
N, m = args.reads, 100
COMP = np.arange(256, dtype=np.uint8)
for a, b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[a] = b


def batch(sub_rate):
    reads, _ = sp.sample_reads(text, info, N, m, seed=20240231, sub_rate=sub_rate)
    r = reads.cpu().numpy().reshape(N, m).copy()
    r[1::2] = COMP[r[1::2, ::-1]]                         # every second read: its reverse complement
    return np.ascontiguousarray(r.reshape(-1))


seq_sets = {s: batch(s) for s in ((args.sub_rate,) if args.trace else (0.0, 0.1))}
del text
torch.cuda.empty_cache()
rb = ra.RowBowt.from_runs(inp["heads"], inp["lens"], inp["ssa"], inp["esa"], device=0)
H = info["H"]
rb.set_docs([f"hap{h}" for h in range(H)], [h * info["unit"] for h in range(H)])
L = ra.lib()
p = capi._p
seq_begin = np.arange(N, dtype=np.uint64) * np.uint64(m)
seq_len = np.full(N, m, dtype=np.uint32)
off = np.arange(N + 1, dtype=np.uint64) * np.uint64(m)
quals = np.full(N * m, ord("I"), dtype=np.uint8)
names = [b"r%d" % i for i in range(N)]
name_len = np.array([len(x) for x in names], dtype=np.uint32)
name_begin = np.concatenate(([0], np.cumsum(name_len[:-1]))).astype(np.uint64)
name_blob = np.frombuffer(b"".join(names), dtype=np.uint8).copy()
del names
lo, hi, k = (np.zeros(N, np.uint64) for _ in range(3))
t0 = time.perf_counter()
rb.fl_prepare()                                           # the FL index of rbg_align_sam_extend_both: once per handle
fl_ms = (time.perf_counter() - t0) * 1e3


def sam(seqs, secondary):
    text_p, n = capi.VP(), capi.U64()
    rc = L.rbg_align_sam(rb.h, p(seqs), p(seq_begin), p(seq_len), p(quals), p(seq_begin), p(name_blob), p(name_begin), p(name_len), N, 20, 16,
                         capi.SAM_SECONDARY if secondary else 0, C.byref(text_p), C.byref(n))
    assert rc == 0, rc
    assert L.rbg_wait_text(rb.h, text_p) == 0
    L.rbg_release_text(rb.h, text_p)
    return n.value


def sam_ext(seqs, secondary):
    text_p, n = capi.VP(), capi.U64()
    rc = L.rbg_align_sam_extend(rb.h, p(seqs), p(seq_begin), p(seq_len), p(quals), p(seq_begin), p(name_blob), p(name_begin), p(name_len), N, 20, 16,
                                capi.SAM_SECONDARY if secondary else 0, args.max_mismatch, C.byref(text_p), C.byref(n))
    assert rc == 0, rc
    assert L.rbg_wait_text(rb.h, text_p) == 0
    L.rbg_release_text(rb.h, text_p)
    return n.value


def sam_both(seqs, secondary):
    text_p, n = capi.VP(), capi.U64()
    rc = L.rbg_align_sam_extend_both(rb.h, p(seqs), p(seq_begin), p(seq_len), p(quals), p(seq_begin), p(name_blob), p(name_begin), p(name_len), N, 20, 16,
                                     capi.SAM_SECONDARY if secondary else 0, args.max_mismatch, C.byref(text_p), C.byref(n))
    assert rc == 0, rc
    assert L.rbg_wait_text(rb.h, text_p) == 0
    L.rbg_release_text(rb.h, text_p)
    return n.value


def report(seqs):
    text_p, n = capi.VP(), capi.U64()
    assert L.rbg_find_range_w_toehold(rb.h, p(seqs), p(off), N, p(lo), p(hi), p(k)) == 0
    rc = L.rbg_align_text(rb.h, p(lo), p(hi), p(k), N, capi.MAXU, 0, p(name_blob), p(name_begin), p(name_len), C.byref(text_p), C.byref(n))
    assert rc == 0, rc
    assert L.rbg_wait_text(rb.h, text_p) == 0
    L.rbg_release_text(rb.h, text_p)
    return n.value


def clock(fn):
    t0 = time.perf_counter()
    nbytes = fn()
    return (time.perf_counter() - t0) * 1e3, nbytes


print(f"sam rate: n={inp['n']} r={inp['r']} {H} documents, {N} reads x {m} bp (half reverse-complemented), min_length 20, max_hits 16, qualities present, "
      f"{args.steps} steps after {args.warmup}", flush=True)
print(json.dumps({"what": "rbg_fl_prepare", "ms": fl_ms, **rb.fl_info()}), flush=True)
if args.trace:
    seqs = seq_sets[args.sub_rate]
    call = sam_both if args.both else sam_ext if args.extend else sam
    ts = [clock(lambda: call(seqs, args.secondary)) for _ in range(args.warmup + args.steps)][args.warmup:]
    print(json.dumps({"what": ("rbg_align_sam_extend_both" if args.both else "rbg_align_sam_extend" if args.extend else "rbg_align_sam") + ", traced (steps synchronised)", "sub_rate": args.sub_rate, "secondary": args.secondary,
                      "ms_median": float(np.median([t for t, _ in ts])), "text_bytes": ts[0][1], "calls": args.warmup + args.steps}), flush=True)
    sys.exit(0)   # (the library prints the split, summed over all the calls above, at exit)
for sub_rate, seqs in seq_sets.items():
    for secondary in (False, True):
        a, x, y, b = [], [], [], []
        for i in range(args.warmup + args.steps):          # the three alternate, call by call
            ta, na = clock(lambda: sam(seqs, secondary))
            tx, nx = clock(lambda: sam_ext(seqs, secondary))
            ty, ny = clock(lambda: sam_both(seqs, secondary))
            tb, nb = clock(lambda: report(seqs))
            if i >= args.warmup:
                y.append(ty)
                a.append(ta)
                x.append(tx)
                b.append(tb)
        for what, ts, nbytes in (("rbg_align_sam", a, na), ("rbg_align_sam_extend", x, nx), ("rbg_align_sam_extend_both", y, ny), ("rbg_find_range_w_toehold + rbg_align_text", b, nb)):
            print(json.dumps({"what": what, "sub_rate": sub_rate, "secondary": secondary if what.startswith("rbg_align_sam") else None,
                              "max_mismatch": args.max_mismatch if what.startswith("rbg_align_sam_extend") else None, "ms_median": float(np.median(ts)),
                              "ms_min": min(ts), "ms_max": max(ts), "text_bytes": nbytes, "reads_per_s": N / (float(np.median(ts)) / 1e3)}), flush=True)
rb.close()
