#!/usr/bin/env python3
"""Milliseconds of the document hits (include/rbg.h: rbg_doc_hits_dev, rbg_doc_hits) on the bench-shaped index with hap<h> documents as bench.py
attaches them, 10 M x 100 bp reads with sub_rate 0.1.  HIP events on the launch stream, --steps steps after --warmup, in one process:
  - rbg_doc_hits_dev over K3's locations of the batch (all four outputs), with the group width chosen on the device and forced to 4, 16 and 64
    (RBG_DOCS_GROUP), and rbg_doc_hits_dev32 over the 32-bit locations; rbg_resolve_offsets_dev over the same locations;
  - K3 (rbg_locate_fill_dev with the chains ordered) on the same batch;
  - a device-to-device hipMemcpyAsync of the same location array: the yardstick -- the copy moves the array twice, the kernel reads it once and
    writes about 1/40 of it, so a kernel slower than the copy has a step to name;
  - end to end on the same reads in pageable host memory (the method of tools/host_api_rate.py): rbg_doc_hits against rbg_find_range_w_toehold +
    rbg_locs_at; and, for the first --check-reads reads, rbg_doc_hits' outputs against the oracle's locations under the lookup rule.
  - rbg_locate_doc_hits_dev (the walk that reduces as it goes, nothing stored per location) with every output, the sets alone, with doc_locs, and with
    d_order NULL, ALTERNATING in the same loop with the two-step sum it replaces -- rbg_locate_plan_dev + rbg_locate_fill_dev + rbg_doc_hits_dev, and the
    32-bit pair rbg_doc_hits takes at 4-byte positions -- median of --steps after --warmup; end to end, rbg_doc_hits with RBG_DOC_HITS_FUSED 0 and 1.
One JSON line per measurement.  GPU box only."""
import argparse
import json
import os
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
ap.add_argument("--H", type=int, default=50, help="haplotypes = documents (bench: 50)")
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--check-reads", type=int, default=20000, help="reads whose rbg_doc_hits outputs are compared with the oracle's (0: none)")
ap.add_argument("--host-calls", type=int, default=3, help="end-to-end calls per entry point (the best is reported); 0 skips them")
args = ap.parse_args()

dev = torch.device("cuda:0")
text, info = sp.make_text(args.L, args.H, 0.01, 20240229, dev)
sa = sp.suffix_array(text)
inp = sp.index_inputs(text, sa)
del sa
N, m = args.reads, 100
reads, _ = sp.sample_reads(text, info, N, m, seed=20240231, sub_rate=0.1)
seqs = reads.cpu().numpy().reshape(-1)
off = np.arange(N + 1, dtype=np.uint64) * np.uint64(m)
del text, reads
torch.cuda.empty_cache()
rb = ra.RowBowt.from_runs(inp["heads"], inp["lens"], inp["ssa"], inp["esa"], device=0)
H = info["H"]
starts = [h * info["unit"] for h in range(H)]
rb.set_docs([f"hap{h}" for h in range(H)], starts)
rb.docs_prepare()
W = rb.doc_hits_words()
L = ra.lib()
st = torch.cuda.current_stream().cuda_stream
MAXU = capi.MAXU


def new(n, dtype=torch.int64):
    return torch.empty(max(n, 1), dtype=dtype, device=dev)


def ok(rc):
    assert rc == 0, rc


def timed(step):
    times = []
    for i in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        if i >= args.warmup:
            times.append(a.elapsed_time(b))
    return float(np.median(times)), min(times), max(times)


d_seqs = torch.from_numpy(np.concatenate([seqs, np.zeros(16, np.uint8)])).to(dev)
d_off = torch.from_numpy(off.view(np.int64)).to(dev)
d_lo, d_hi, d_k, d_loc_off = new(N), new(N), new(N), new(N + 1)
ok(L.rbg_find_range_w_toehold_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, d_lo.data_ptr(), d_hi.data_ptr(), d_k.data_ptr(), st))
tmp_bytes, ws_bytes = L.rbg_locate_plan_tmp_bytes(N), L.rbg_locate_order_ws_bytes(N)
d_tmp, d_ws = new(tmp_bytes, torch.uint8), new(ws_bytes, torch.uint8)
ok(L.rbg_locate_plan_dev(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), N, MAXU, d_loc_off.data_ptr(), d_tmp.data_ptr(), tmp_bytes, st))
total = int(d_loc_off[-1].item())
d_locs, d_copy = new(total), new(total)
ok(L.rbg_locate_order_dev(rb.h, d_k.data_ptr(), N, d_ws.data_ptr(), ws_bytes, st))
print(f"document hits: n={inp['n']} r={inp['r']} {H} documents (W = {W}), {N} reads x {m} bp, {total} locations ({total / N:.1f} per read, "
      f"{total * 8 / 1e9:.2f} GB), {args.steps} steps after {args.warmup}", flush=True)
rows = {}


def k3():
    ok(L.rbg_locate_fill_dev(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), d_k.data_ptr(), N, MAXU, d_loc_off.data_ptr(), d_locs.data_ptr(), d_ws.data_ptr(), st))


rows["K3: rbg_locate_fill_dev, chains ordered"] = timed(k3)
d_sets, d_nd, d_no, d_dr = new(N * W), new(N, torch.int32), new(N, torch.int32), torch.zeros(H, dtype=torch.int64, device=dev)


def hits():
    ok(L.rbg_doc_hits_dev(rb.h, d_locs.data_ptr(), d_loc_off.data_ptr(), N, d_sets.data_ptr(), d_nd.data_ptr(), d_no.data_ptr(), d_dr.data_ptr(), st))


for group in ("", "4", "16", "64"):
    if group:
        os.environ["RBG_DOCS_GROUP"] = group   # (read by the library at every launch)
    else:
        os.environ.pop("RBG_DOCS_GROUP", None)
    rows[f"rbg_doc_hits_dev, group {'chosen on the device' if not group else group}"] = timed(hits)
os.environ.pop("RBG_DOCS_GROUP", None)
rows["rbg_doc_hits_dev, sets only"] = timed(lambda: ok(L.rbg_doc_hits_dev(rb.h, d_locs.data_ptr(), d_loc_off.data_ptr(), N, d_sets.data_ptr(), None, None, None, st)))
d_doc = new(total, torch.int32)
rows["rbg_resolve_offsets_dev, documents only"] = timed(lambda: ok(L.rbg_resolve_offsets_dev(rb.h, d_locs.data_ptr(), total, d_doc.data_ptr(), None, st)))
del d_doc


def hip_runtime():
    """the HIP runtime this process already runs (one per process: rowbowt_amd/capi.py _one_hip_runtime)"""
    import ctypes
    for line in open("/proc/self/maps"):
        if "libamdhip64.so" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no libamdhip64 mapped")


hip = hip_runtime()
hip.hipMemcpyAsync.argtypes = [capi.VP, capi.VP, capi.C.c_size_t, capi.C.c_int, capi.VP]
rows["device-to-device hipMemcpyAsync of the locations"] = timed(lambda: ok(hip.hipMemcpyAsync(d_copy.data_ptr(), d_locs.data_ptr(), total * 8, 3, st)))   # 3 = hipMemcpyDeviceToDevice
if rb.info().pos_bytes == 4:
    d_locs32 = new(total, torch.int32)
    ok(L.rbg_locate_fill_dev32(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), d_k.data_ptr(), N, MAXU, d_loc_off.data_ptr(), d_locs32.data_ptr(), d_ws.data_ptr(), st))
    rows["rbg_doc_hits_dev32"] = timed(lambda: ok(L.rbg_doc_hits_dev32(rb.h, d_locs32.data_ptr(), d_loc_off.data_ptr(), N, d_sets.data_ptr(), d_nd.data_ptr(),
                                                                       d_no.data_ptr(), d_dr.data_ptr(), st)))
    del d_locs32
for what, (med, lo_, hi_) in rows.items():
    print(json.dumps({"step": what, "ms_median": round(med, 4), "ms_min": round(lo_, 4), "ms_max": round(hi_, 4), "reads": N, "locations": total,
                      "GBps_of_locations": round(total * 8 / (med * 1e-3) / 1e9, 1)}), flush=True)
copy_ms, hit_ms = rows["device-to-device hipMemcpyAsync of the locations"][0], rows["rbg_doc_hits_dev, group chosen on the device"][0]
print(json.dumps({"rbg_doc_hits_dev / copy of the locations": round(hit_ms / copy_ms, 3), "rbg_doc_hits_dev / K3": round(hit_ms / rows["K3: rbg_locate_fill_dev, chains ordered"][0], 3)}),
      flush=True)

# ---- the fused walk against the two-step sum, alternating in one loop: the same (lo, hi, k), the same order workspace, the same outputs ----
d_dl = torch.zeros(H, dtype=torch.int64, device=dev)
d_sets2, d_nd2, d_no2, d_dr2 = new(N * W), new(N, torch.int32), new(N, torch.int32), torch.zeros(H, dtype=torch.int64, device=dev)
pos32 = rb.info().pos_bytes == 4
d_locs32 = new(total, torch.int32) if pos32 else None


def two_step():
    ok(L.rbg_locate_plan_dev(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), N, MAXU, d_loc_off.data_ptr(), d_tmp.data_ptr(), tmp_bytes, st))
    k3()
    hits()


def two_step32():
    ok(L.rbg_locate_plan_dev(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), N, MAXU, d_loc_off.data_ptr(), d_tmp.data_ptr(), tmp_bytes, st))
    ok(L.rbg_locate_fill_dev32(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), d_k.data_ptr(), N, MAXU, d_loc_off.data_ptr(), d_locs32.data_ptr(), d_ws.data_ptr(), st))
    ok(L.rbg_doc_hits_dev32(rb.h, d_locs32.data_ptr(), d_loc_off.data_ptr(), N, d_sets.data_ptr(), d_nd.data_ptr(), d_no.data_ptr(), d_dr.data_ptr(), st))


def fused(order=True, counts=True, locs=False):
    def run():
        ok(L.rbg_locate_doc_hits_dev(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), d_k.data_ptr(), N, MAXU, d_ws.data_ptr() if order else None, d_sets2.data_ptr(),
                                     d_nd2.data_ptr() if counts else None, d_no2.data_ptr() if counts else None, d_dr2.data_ptr() if counts else None,
                                     d_dl.data_ptr() if locs else None, st))
    return run


ab = {"two-step: rbg_locate_plan_dev + rbg_locate_fill_dev + rbg_doc_hits_dev": two_step}
if pos32:
    ab["two-step, 32-bit locations: plan + rbg_locate_fill_dev32 + rbg_doc_hits_dev32"] = two_step32
ab["rbg_locate_doc_hits_dev, every output but doc_locs, ordered"] = fused()
ab["rbg_locate_doc_hits_dev, sets only, ordered"] = fused(counts=False)
ab["rbg_locate_doc_hits_dev, every output with doc_locs, ordered"] = fused(locs=True)
ab["rbg_locate_doc_hits_dev, every output but doc_locs, d_order NULL"] = fused(order=False)
ab_ms = {what: [] for what in ab}
for i in range(args.warmup + args.steps):
    for what, step in ab.items():   # (alternating: every row sees the same clocks and the same neighbours)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        if i >= args.warmup:
            ab_ms[what].append(a.elapsed_time(b))
for what, t in ab_ms.items():
    print(json.dumps({"step": what, "ms_median": round(float(np.median(t)), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "reads": N, "locations": total}),
          flush=True)
torch.cuda.synchronize()
same = bool((d_sets2 == d_sets).all().item() and (d_nd2 == d_nd).all().item() and (d_no2 == d_no).all().item())
base = min(float(np.median(t)) for what, t in ab_ms.items() if what.startswith("two-step"))
fused_ms = float(np.median(ab_ms["rbg_locate_doc_hits_dev, every output but doc_locs, ordered"]))
spread = max(max(t) - min(t) for what, t in ab_ms.items() if what.startswith("two-step"))
print(json.dumps({"fused / two-step (the faster two-step row)": round(fused_ms / base, 3), "two-step spread ms": round(spread, 4),
                  "fused outputs equal the two-step outputs": same}), flush=True)
assert same
del d_copy, d_locs, d_sets, d_seqs, d_sets2, d_locs32
torch.cuda.empty_cache()

if args.host_calls > 0:
    best_hits = best_locs = 1e9
    # the A/B switch of the host call, the two-step path against the fused one, ALTERNATING call by call after one call of each that is not counted: calls
    # later in a process run slower than the first ones whatever they are (the rows below come out 10 % above a fresh process's)
    ab_s = {"0": [], "1": []}
    for rep in range(args.host_calls + 1):
        for fused_env in ("0", "1"):
            os.environ["RBG_DOC_HITS_FUSED"] = fused_env
            t0 = time.perf_counter()
            lo, hi, sets, ndocs, nodoc, doc_reads = rb.doc_hits(seqs, off)
            if rep:
                ab_s[fused_env].append(time.perf_counter() - t0)
    os.environ.pop("RBG_DOC_HITS_FUSED", None)
    for fused_env, t in ab_s.items():
        print(json.dumps({"end to end, pageable host memory": f"rbg_doc_hits, RBG_DOC_HITS_FUSED={fused_env}", "s": round(min(t), 4), "s_all": [round(x, 4) for x in t],
                          "reads_per_s": N / min(t)}), flush=True)
    for _ in range(args.host_calls):
        t0 = time.perf_counter()
        lo, hi, sets, ndocs, nodoc, doc_reads = rb.doc_hits(seqs, off)
        best_hits = min(best_hits, time.perf_counter() - t0)
    for _ in range(args.host_calls):
        t0 = time.perf_counter()
        lo2, hi2, k2 = rb.find_range_w_toehold(seqs, off)
        loc_off, locs = rb.locs_at(lo2, hi2, k2)
        best_locs = min(best_locs, time.perf_counter() - t0)
    back = 16 + 8 * W + 8
    print(json.dumps({"end to end, pageable host memory": "rbg_doc_hits", "s": round(best_hits, 4), "reads_per_s": N / best_hits, "bytes_back_per_read": back}), flush=True)
    print(json.dumps({"end to end, pageable host memory": "rbg_find_range_w_toehold + rbg_locs_at", "s": round(best_locs, 4), "reads_per_s": N / best_locs,
                      "bytes_back_per_read": round(24 + 8 + 8 * len(locs) / N, 1)}), flush=True)
    assert (lo == lo2).all() and (hi == hi2).all()
    # rbg_doc_hits' outputs for the first --check-reads reads against the oracle: its locs_at_batch, and the lookup rule as tests/doc_hits_model.py states it
    # (that model is checked against the oracle's resolve_offset by tests/test_doc_hits_model.py)
    nchk = min(args.check_reads, N)
    if nchk:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import doc_hits_model  # noqa: E402
        import orc  # noqa: E402
        o = orc.Oracle.from_runs(inp["heads"], inp["lens"], inp["ssa"], inp["esa"])
        ncpu = min(os.cpu_count() or 1, 16)
        h_off = off[:nchk + 1]
        wlo, whi, wk = o.find_range_w_toehold_batch(seqs[:nchk * m], h_off, nthreads=ncpu)
        woff, wlocs = o.locs_at_batch(wlo, whi, wk, MAXU, nthreads=ncpu)
        wsets, wnd, wno, _ = doc_hits_model.doc_hits(wlocs, woff, starts)
        same = bool((sets[:nchk] == wsets).all() and (ndocs[:nchk] == wnd).all() and (nodoc[:nchk] == wno).all() and (lo[:nchk] == wlo).all() and (hi[:nchk] == whi).all())
        print(json.dumps({"reads checked against the oracle": nchk, "locations": int(woff[-1]), "sets, ndocs, nodoc and ranges equal": same,
                          "reads per document (first 5)": doc_reads[:5].tolist()}), flush=True)
        o.close()
        assert same
rb.close()
