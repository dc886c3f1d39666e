"""CPU check of the marker directory (rbg_mkdir.hpp: the shift rule, the gates, the bucket-record builder of upload_marker_table and the record arithmetic of
marker_query) at the bucket widths, row offsets, value counts and value offsets that no index of test size reaches."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_marker_directory_against_a_scan_over_the_runs(tmp_path):
    """tests/cpp/mkrec_check.cpp under ASan + UBSan.  Tables built with the real builder, every query answered through the records, through the directory and the
    arrays, and by binary search, each {first run, one past the last, first value, number of values} against a scan over the runs: forced shifts 0, 1, 8, 14, 15,
    16, 17 and 20 (no records from 17 on); at shift 16 run ends on F + 0xFFFE / 0xFFFF / 0x10000 / 0x2FFFF, starts on F, F + 1 and F + 0xFFFF, a run from before F,
    a run over three whole buckets, buckets listing 0, 1, 3 and 4 runs, runs of 0, 1, 65535 and 65536 values, with lo and hi on each of those rows, their
    neighbours, both ends of every bucket, n - 1, n and n + 5; value offsets across 2^32 inside one record and up to 2^40 - 1; 4000 fixed-seed tables of shifts
    0..16.  The gates at the values where they flip, the shift rule on both sides of each threshold of the shifts 14..20 and at the (n, nruns) of
    test_gpu_marker_dir.py.  The line asserted is the number of comparisons per path: a case that stops reaching its path changes it."""
    exe = tmp_path / "mkrec"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "mkrec_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, timeout=300)
    assert p.returncode == 0 and b"mkrec ok records 321888 overflow 44924 directory 396058 bsearch 396058\n" == p.stdout, p.stdout[-300:] + p.stderr[-600:]
