"""CPU check of the decimals the text kernels write (rbg_text_dev.hpp dec_len / put_dec, shared by k_text.hip and k_report.hip)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dec_len_and_put_dec_against_snprintf(tmp_path):
    """tests/cpp/text_dec_check.cpp under ASan + UBSan: 0, 10^k - 1 / 10^k / 10^k + 1 for k = 1..19, 2^k - 1 / 2^k for k = 1..63, 2^64 - 1 and
    100 000 fixed-seed values over all widths; the length against snprintf's, the digits against its bytes, sentinels on both sides of the
    digits intact after every call"""
    exe = tmp_path / "text_dec"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "text_dec_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, timeout=300)
    assert p.returncode == 0 and b"text dec ok 100185" in p.stdout, p.stdout[-300:] + p.stderr[-300:]
