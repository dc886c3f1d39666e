"""CPU check of the ISA sample that host and device share (rowbowt_amd/csrc/rbg_isa.hpp: builder, directory, lookup, the row of a position)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_isa_sample_on_the_host(tmp_path):
    """tests/cpp/isa_check.cpp, a stand-alone program with its own main under ASan + UBSan, run directly: isa_build from the run arrays and toehold samples of
    small texts and isa_lookup / isa_row at every position against a naive ISA at both position widths, with each shape asserted present in the inputs
    (shift == 0, a bucket that holds no sample, a bucket that needs the bisection, the first and last positions, a row inside a run of a symbol that is no
    base, a non-base BWT run of at least 16 rows and two non-base bytes side by side in the text: a collection of 40 near-copy documents with '#', runs of N,
    "N#", "##" and a leading N); 8-byte positions over a synthetic sample list with samples on both sides of 2^32, lookup only; what the builder refuses."""
    exe = tmp_path / "isa_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "isa_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith(b"isa host ok ") and p.stdout.count(b"\n") == 1, p.stdout[-300:] + p.stderr[-600:]
    assert int(p.stdout.split()[3]) >= 10000
