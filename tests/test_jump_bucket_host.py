"""CPU check of the jump table's bucket decision (rbg_jump.h jump_bucket) and of jump_probe expressed over it, on host-built tables."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jump_bucket_and_probe_against_a_linear_scan(tmp_path):
    """tests/cpp/jump_bucket_check.cpp under ASan + UBSan: tables of 1, 2, 3 and 8 buckets; chains that wrap from the last bucket to
    bucket 0, a key in slot 1 behind another key in slot 0, an absent key whose chain ends at an empty slot 1, an absent key in a table
    without an empty slot (the nb-bucket bound); every answer and bucket count against a linear scan of the table"""
    exe = tmp_path / "jump_bucket"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "jump_bucket_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, timeout=300)
    assert p.returncode == 0 and b"jump bucket ok" in p.stdout, p.stdout[-300:] + p.stderr[-300:]
