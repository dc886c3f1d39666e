"""CPU check of the left-extension rules that host and device share (rowbowt_amd/csrc/rbg_sam.hpp: the walk, MD, the extended line's length and bytes)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extension_rules_on_the_host(tmp_path):
    """tests/cpp/sam_extend_host_check.cpp, a stand-alone program with its own main under ASan + UBSan, run directly: sam_extend_begin / sam_extend_take against the
    rule written out again over 4 000 random flanks at K = 0 .. 8 (limits below, at and beyond the prefix; terminators and N in the reference; N and lower
    case in the read; mismatches at the first and the last extended base; walks ended by the budget, by a base, by the length; trimmed mismatches);
    sam_line_len == the bytes sam_put_line writes == a line put together from strings, with sentinels on both sides, for extension records with MD numbers
    of 1 to 3 digits and a POS that loses a digit, primary and secondary lines of both strands, with and without qualities, and without a record
    (rbg_align_sam's line).  The line asserted carries the number of checks, with a lower bound."""
    exe = tmp_path / "sam_extend_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "sam_extend_host_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith(b"sam extend host ok ") and p.stdout.count(b"\n") == 1, p.stdout[-300:] + p.stderr[-600:]
    assert int(p.stdout.split()[4]) >= 700000
