#!/usr/bin/env python3
"""Marker-array construction rate: rbg_marker_runs_plan_dev + rbg_marker_runs_fill_dev (rowbowt_amd/csrc/mk_build.hip, through capi.marker_runs) against
synth_pangenome.marker_array, the torch model that goes through an inverse suffix array, on synth_pangenome.make_text at the bench shape (bench.py's default
L, H, site_rate) or the shape given, with windows of w = 10.  Where the shape does not fit the device -- 96 bytes per symbol are asked for, as tools/sa_rate.py
asks for the suffix-array builders -- L is halved until it does, and the output states the shape that ran.

The site records are the ones marker_array infers from the text: a site is a column where some haplotype differs from the first, every haplotype copy
carries one record per site (allele 1 where it differs), the window is clipped where the copy starts.  One process, the two builders alternating on the
same suffix array (capi.suffix_array): 1 warm-up and 5 timed runs each (wall time around a device synchronisation; the copy of the four arrays to the
host is inside both), median and range.  The four arrays are ASSERTED equal.  Peak device bytes of each beside the text, the suffix array and the records: the peak of
torch's allocator above its value before the call (both builders allocate through it), and the fall of hipMemGetInfo's free bytes below its value right
before the call, polled every 2 ms (the driver may count blocks freed by earlier calls as used for a while, which hides allocations from this figure).  The structural claim of DESIGN 6l is ASSERTED:
rbg_marker_runs_tmp_bytes < n + 64 S w.  Also, once: rb_build --fasta --vcf -m -s -l end to end on a FASTA (the first haplotype) and a VCF (the others as
haploid samples) written from the text.

    python tools/marker_build_rate.py [--L 40000000 --H 50 --site-rate 0.01] [--w 10] [--out profiles/marker_build_rate.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rowbowt_amd import capi  # noqa: E402
from rowbowt_amd.tools import synth_pangenome as SP  # noqa: E402
from sa_rate import BYTES_PER_SYMBOL, LowWater  # noqa: E402


def timed(fn):
    """-> (result, seconds, fall of hipMemGetInfo's free bytes below its value right before the call, peak bytes of torch's allocator above its
    value right before the call): both builders allocate through torch, so the second is exact where the driver reports freed blocks late"""
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held, free = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0]
    with LowWater() as lw:
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return out, dt, free - lw.low, torch.cuda.max_memory_allocated() - held


def site_records(text, info, w):
    """(pos, first, val) int64 on the device, ascending in pos, and the sites and the alleles [H, sites] they were made from"""
    unit, H, L = info["unit"], info["H"], info["L"]
    haps = text[:H * unit].view(H, unit)[:, :L]
    sites = torch.nonzero((haps != haps[0][None, :]).any(dim=0)).flatten()
    allele = (haps[:, sites] != haps[0][sites][None, :]).to(torch.int64)
    start = (torch.arange(H, device=text.device, dtype=torch.int64) * unit)[:, None]
    pos = start + sites[None, :]
    first = torch.maximum(start.expand_as(pos), pos - (w - 1))
    val = sites[None, :] | (allele << 60)
    return pos.flatten().contiguous(), first.flatten().contiguous(), val.flatten().contiguous(), sites, allele


def write_inputs(d, text, info, sites, allele):
    """ref.fa = the first haplotype; calls.vcf = the other haplotypes as haploid samples h1 .. h(H-1)"""
    unit, H, L = info["unit"], info["H"], info["L"]
    host = text.cpu().numpy()
    with open(os.path.join(d, "ref.fa"), "wb") as f:
        f.write(b">ref\n" + host[:L].tobytes() + b"\n")
    s = sites.cpu().numpy()
    ref = host[s]
    alt = np.zeros(len(s), np.uint8)
    al = allele.cpu().numpy()
    for h in range(1, H):      # (one ALT per site: the base of a haplotype that differs)
        b = host[h * unit + s]
        alt = np.where((alt == 0) & (b != ref), b, alt)
    with open(os.path.join(d, "calls.vcf"), "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"h{h}" for h in range(1, H)) + "\n")
        for k in range(len(s)):
            f.write(f"ref\t{int(s[k]) + 1}\t.\t{chr(ref[k])}\t{chr(alt[k])}\t.\t.\t.\tGT\t" + "\t".join(str(int(al[h, k])) for h in range(1, H)) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=40_000_000)
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--site-rate", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=20240229)
    ap.add_argument("--w", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    asked_L = a.L
    free0 = torch.cuda.mem_get_info()[0]
    while a.L > 1000 and (a.H * (a.L + 10) + 1) * BYTES_PER_SYMBOL > free0:
        a.L //= 2
    text, info = SP.make_text(a.L, a.H, a.site_rate, a.seed, "cuda")
    n = info["n"]
    if a.L != asked_L:
        say(f"L = {asked_L} asked for: {(a.H * (asked_L + 10) + 1) * BYTES_PER_SYMBOL} bytes do not fit the {free0} free; L halved to {a.L}, the largest such shape that fits")
    say(f"shape: make_text(L={a.L}, H={a.H}, site_rate={a.site_rate}, seed={a.seed}): n = {n} symbols, w = {a.w}; bench.py's default shape is L=40000000, H=50, site_rate=0.01")
    sa = capi.suffix_array(text)
    sa64 = sa.to(torch.int64)      # (marker_array indexes with it)
    pos, first, val, sites, allele = site_records(text, info, a.w)
    S, pb = int(pos.numel()), sa.element_size()
    tmp = int(capi.lib().rbg_marker_runs_tmp_bytes(n, S, a.w, pb))
    say(f"records: {int(sites.numel())} sites x {a.H} haplotype copies = S = {S}; {pb}-byte positions")
    say(f"rbg_marker_runs_tmp_bytes = {tmp} = {tmp / n:.4f} per symbol ({(tmp - 32 * min(n, S * a.w)) / n:.4f} without the 32 bytes per row that can be covered); "
        f"the bound n + 64 S w = {n + 64 * S * a.w}")
    assert 0 < tmp < n + 64 * S * a.w, (tmp, n, S, a.w)
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    base_free = torch.cuda.mem_get_info()[0]
    say(f"device: {torch.cuda.get_device_name(0)}, {torch.cuda.mem_get_info()[1]} bytes, {base_free} free with the text, both suffix arrays and the records resident")
    t_new, t_ref, p_new, p_ref, a_new, a_ref = [], [], [], [], [], []
    for it in range(a.runs + 1):
        got, dt, peak, alloc = timed(lambda: capi.marker_runs(sa, pos, first, val, a.w))
        if it:
            t_new.append(dt), p_new.append(peak), a_new.append(alloc)
        want, dt, peak, alloc = timed(lambda: SP.marker_array(text, info, sa64, a.w))
        if it:
            t_ref.append(dt), p_ref.append(peak), a_ref.append(alloc)
        for name, x, y in zip(("run_start", "run_end", "mk_off", "mk_vals"), got, want):
            assert x.shape == y.shape and bool((x == y).all()), (name, it, x.shape, y.shape)
    say(f"arrays equal in all {a.runs + 1} rounds: {len(got[0])} runs, {len(got[3])} values")
    for what, t, p, al in (("rbg_marker_runs_plan_dev + fill_dev", t_new, p_new, a_new), ("synth_pangenome.marker_array (torch)", t_ref, p_ref, a_ref)):
        say(f"{what}: median {statistics.median(t):.3f} s (range {min(t):.3f} .. {max(t):.3f}, {len(t)} runs after 1), {n / statistics.median(t) / 1e6:.1f} M symbols/s; "
            f"peak device bytes beside the text, the suffix array and the records (result included): {max(al)} = {max(al) / n:.3f} per symbol by torch's allocator, "
            f"through which both allocate; low-water mark of hipMemGetInfo below its value right before the call {max(p)} = {max(p) / n:.3f} per symbol")
    say(f"ratio of the medians, torch / device pass: {statistics.median(t_ref) / statistics.median(t_new):.2f}")
    if not a.no_cli:
        with tempfile.TemporaryDirectory() as d:
            write_inputs(d, text, info, sites, allele)
            t0 = time.perf_counter()
            p = subprocess.run([os.path.join(ROOT, "rowbowt_amd", "rb_build"), "--fasta", os.path.join(d, "ref.fa"), "--vcf", os.path.join(d, "calls.vcf"), "--ma-wsize",
                                str(a.w), "-m", "-s", "-l", "-o", os.path.join(d, "x")], capture_output=True)
            dt = time.perf_counter() - t0
            say(f"rb_build --fasta --vcf -m -s -l end to end (1 contig of {a.L} bases, {int(sites.numel())} VCF lines of {a.H - 1} haploid samples; process start, parse, "
                f"upload, build, cache write): {dt:.2f} s, exit {p.returncode}, cache {os.path.getsize(os.path.join(d, 'x.rbgpu')) if p.returncode == 0 else 0} bytes")
            if p.returncode:
                say("  stderr: " + p.stderr.decode()[-300:].replace("\n", " | "))
    say("not measured: n >= 2^32 (8-byte positions at their real size); hardware counters")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
