"""CPU check of the FL index that host and device share (rowbowt_amd/csrc/rbg_fl.hpp: builder, directory, step) and of the formatter with two extension
records (rowbowt_amd/csrc/rbg_sam.hpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fl_index_on_the_host(tmp_path):
    """tests/cpp/fl_check.cpp, a stand-alone program with its own main under ASan + UBSan, run directly: fl_build and fl_step at every row of small BWTs at
    both position widths against select over the expanded BWT, with each shape asserted present in the inputs (a base with a single run, an absent base,
    shift == 0, a bucket of 2^shift one-symbol runs, a run over several buckets, the first and last row of each base's F interval, rows of the terminator
    and of a separator, a bucket that is searched); 8-byte positions over runs whose lengths carry rows across 2^32 against the arithmetic written out
    again; sam_line_len == the bytes sam_put_line writes with two records, MD starting and ending with a number and re-expanding to both flanks."""
    exe = tmp_path / "fl_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "fl_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith(b"fl host ok ") and p.stdout.count(b"\n") == 1, p.stdout[-300:] + p.stderr[-600:]
    assert int(p.stdout.split()[3]) >= 100000
