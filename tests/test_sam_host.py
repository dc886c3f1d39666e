"""CPU check of the SAM rules that host and device share (rowbowt_amd/csrc/rbg_sam.hpp: complement, CIGAR, line length and formatter, header text)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sam_rules_on_the_host(tmp_path):
    """tests/cpp/sam_host_check.cpp, a stand-alone program under ASan + UBSan: the complement over all 256 bytes (an involution on ACGTacgt, the identity
    elsewhere); CIGAR text and length for a and m - b in {0, 1, 9, 10} and b - a at 10^k and 10^k - 1, k = 0 .. 19; sam_line_len == the bytes sam_put_line
    writes == a line put together from strings, with sentinels on both sides of the buffer -- unmapped, primary and secondary lines of both strands, with and
    without qualities, names of 0, 1 and 300 bytes, decimals up to 2^64 - 1; the header for 1, 2 and 1 024 documents, names of length 0 and 300, unsorted
    input starts, a last start beyond n.  The line asserted carries the number of checks, with a lower bound: a loop that stops running falls below it."""
    exe = tmp_path / "sam_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "sam_host_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith(b"sam host ok ") and p.stdout.count(b"\n") == 1, p.stdout[-300:] + p.stderr[-600:]
    assert int(p.stdout.split()[3]) >= 3925          # (what the cases above come to; more cases only raise it)
