"""rowbowt_gpu.hpp's doc_hits overloads with doc_locs, instantiated and run (tests/cpp/locate_doc_hits_shim_check.cpp), against the oracle's
locs_at_batch reduced by the numpy model; in the manner of test_gpu_doc_hits.test_cpp_shim_doc_hits_and_resolve_offsets."""
import os
import subprocess

import pytest

import orc
import rowbowt_amd as ra
from test_gpu_locate_doc_hits import MAXU, model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_shim_doc_hits_with_doc_locs(data_dir, tmp_path, simple_reads, error_reads):
    o = orc.Oracle.load(os.path.join(data_dir, "small.fa"), orc.SA)
    exe = tmp_path / "locate_doc_hits_shim_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rowbowt_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "locate_doc_hits_shim_check.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "rowbowt_amd"), "-lrbg", "-Wl,-rpath," + os.path.join(ROOT, "rowbowt_amd")])
    reads = [r for r in (simple_reads + error_reads) if r and b"\n" not in r][:40] + [b"AC", b"ACG", b"TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT"]
    qfile = tmp_path / "q.txt"
    qfile.write_bytes(b"\n".join(reads) + b"\n")
    seqs, off = ra.pack_reads(reads)
    wlo, whi, wk = o.find_range_w_toehold_batch(seqs, off)
    for starts, max_hits in (([20000, 0, 25000, 5000, 12000], MAXU), ([0, 3000, 9000, 21000], 3), ([17, 4000], MAXU)):
        p = subprocess.run([str(exe), os.path.join(data_dir, "small.fa"), str(qfile), str(max_hits), ",".join(map(str, starts))], capture_output=True, timeout=300)
        assert p.returncode == 0, p.stdout.decode()[-500:] + p.stderr.decode()[-2000:]
        woff, wlocs = o.locs_at_batch(wlo, whi, wk, max_hits)
        want = model(wlocs, woff, starts)
        lines = [f"read {int(wlo[i])} {int(whi[i])} {int(want['ndocs'][i])} {int(want['nodoc'][i])} " + " ".join(str(int(w)) for w in want["sets"][i])
                 for i in range(len(reads))]
        lines.append(" ".join(["reads"] + [str(int(c)) for c in want["doc_reads"]]))
        lines.append(" ".join(["locs"] + [str(int(c)) for c in want["doc_locs"]]))
        lines.append("same 1")
        assert p.stdout.decode().splitlines() == lines, starts
        assert int(want["doc_locs"].sum()) + int(want["nodoc"].sum()) == len(wlocs) and int(want["doc_locs"].max()) >= 2
    o.close()
