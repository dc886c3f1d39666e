#!/usr/bin/env python3
"""Suffix-array construction rate: rbg_suffix_array_dev (rowbowt_amd/csrc/sa_build.hip) against synth_pangenome.suffix_array, the torch prefix doubling
bench.py builds its index with, on synth_pangenome.make_text at the bench shape (bench.py's default L, H, site_rate) or the shape given.  Where that
shape does not fit the device for BOTH builders -- 96 bytes per symbol are asked for: the torch path's measured 85 beside the text, the text, and room to
spare -- L is halved until it does, and the first line of the output states the shape that ran and the one that was asked for.

One process, the two builders alternating: 1 warm-up and 5 timed runs each (wall time around a device synchronisation), median and range.  The arrays are
compared element by element.  Peak device bytes of each = the fall of hipMemGetInfo's free bytes below its value with only the text resident, polled by a
thread every 2 ms (torch's caching allocator is emptied before every run, so its cached blocks are not counted for the other side).  Also, once each:
rbg_text_runs on the result, and rb_build --fasta end to end on a FASTA written from the text.  What is not measured is stated in the output.

    python tools/sa_rate.py [--L 40000000 --H 50 --site-rate 0.01] [--out profiles/sa_build_rate.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rowbowt_amd import capi  # noqa: E402
from rowbowt_amd.tools import synth_pangenome as SP  # noqa: E402


BYTES_PER_SYMBOL = 96      # what a shape must leave room for: the torch path's peak (85 per symbol in profiles/sa_build_rate.txt), the text, a margin


class LowWater:
    """the lowest free device memory seen while the block runs"""

    def __enter__(self):
        self.low = torch.cuda.mem_get_info()[0]
        self.stop = False
        self.t = threading.Thread(target=self._poll)
        self.t.start()
        return self

    def _poll(self):
        while not self.stop:
            self.low = min(self.low, torch.cuda.mem_get_info()[0])
            time.sleep(0.002)

    def __exit__(self, *exc):
        self.stop = True
        self.t.join()
        self.low = min(self.low, torch.cuda.mem_get_info()[0])


def timed(fn, base_free):
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    with LowWater() as lw:
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return out, dt, base_free - lw.low


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=40_000_000)
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--site-rate", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=20240229)
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
        say(f"L = {asked_L} asked for: {(a.H * (asked_L + 10) + 1) * BYTES_PER_SYMBOL} bytes for both builders do not fit the {free0} free; L halved to {a.L}, the largest such shape that fits")
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    base_free = torch.cuda.mem_get_info()[0]
    say(f"shape: make_text(L={a.L}, H={a.H}, site_rate={a.site_rate}, seed={a.seed}): n = {n} symbols; bench.py's default shape is L=40000000, H=50, site_rate=0.01")
    say(f"device: {torch.cuda.get_device_name(0)}, {torch.cuda.mem_get_info()[1]} bytes, {base_free} free with the text resident")
    t_new, t_ref, p_new, p_ref = [], [], [], []
    same = None
    for it in range(a.runs + 1):
        sa_new, dt, peak = timed(lambda: capi.suffix_array(text), base_free)
        inf = capi.sa_info()
        if it:
            t_new.append(dt), p_new.append(peak)
        sa_ref, dt, peak = timed(lambda: SP.suffix_array(text), base_free)
        if it:
            t_ref.append(dt), p_ref.append(peak)
        if same is None:
            same = bool((sa_new.to(torch.int64) == sa_ref).all())
        del sa_ref
        if it < a.runs:
            del sa_new
    say(f"arrays equal: {same}")
    for what, t, p in (("rbg_suffix_array_dev", t_new, p_new), ("synth_pangenome.suffix_array (torch)", t_ref, p_ref)):
        say(f"{what}: median {statistics.median(t):.3f} s (range {min(t):.3f} .. {max(t):.3f}, {len(t)} runs after 1), {n / statistics.median(t) / 1e6:.1f} M symbols/s; "
            f"peak device bytes beside the text {max(p)} = {max(p) / n:.1f} per symbol (result included)")
    say(f"rbg_sa_info: rounds {inf['rounds']}, elements sorted {inf['sorted']} = {inf['sorted'] / n:.2f} n, scratch {inf['tmp_bytes']} bytes = {inf['tmp_bytes'] / n:.1f} per symbol, "
        f"{inf['pos_bytes']}-byte positions, {inf['tied_after_first']} suffixes tied after the first key")
    say("torch path: one round per doubling from 4 symbols, every round sorts n int64 keys with int64 indices")
    runs, dt, _ = timed(lambda: capi.text_runs(text, sa_new), base_free)
    say(f"rbg_text_runs (plan + fill + copy of the run arrays): {dt:.3f} s, r = {runs['r']}")
    if not a.no_cli:
        with tempfile.TemporaryDirectory() as d:
            host = text.cpu().numpy()
            unit, L = info["unit"], info["L"]
            with open(os.path.join(d, "ref.fa"), "wb") as f:
                for h in range(a.H):
                    f.write(b">hap%d\n" % h)
                    f.write(host[h * unit:h * unit + L].tobytes())
                    f.write(b"\n")
            t0 = time.perf_counter()
            p = subprocess.run([os.path.join(ROOT, "rowbowt_amd", "rb_build"), "--fasta", os.path.join(d, "ref.fa"), "-s", "-l", "-o", os.path.join(d, "ref")],
                               capture_output=True)
            dt = time.perf_counter() - t0
            say(f"rb_build --fasta -s -l end to end ({a.H} records of {L} bases, one line each; process start, parse, upload, build, cache write): {dt:.2f} s, exit {p.returncode}, "
                f"cache {os.path.getsize(os.path.join(d, 'ref.rbgpu')) if p.returncode == 0 else 0} bytes")
    say("not measured: n >= 2^32 (8-byte positions at their real size; the 8-byte path is tested on small texts only); hardware counters")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
