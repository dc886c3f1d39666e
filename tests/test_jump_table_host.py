"""CPU checks of the jump table (rbg_jump.h): key packing and probe termination on a host model of the table, and the option's range."""
import os
import subprocess

import rowbowt_amd as ra
from rowbowt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jump_key_packing_and_probe_termination(tmp_path):
    """tests/cpp/jump_table_check.cpp under ASan + UBSan: keys from the staged / packed layout, masking beyond K, a full bucket
    chain, wrap-around at the table's end, absent keys sharing a home bucket, keys that differ only in their last symbol"""
    exe = tmp_path / "jump_table"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "jump_table_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, timeout=300)
    assert p.returncode == 0 and b"jump table ok" in p.stdout, p.stdout[-300:] + p.stderr[-300:]


def test_jump_k_option_range():
    """RBG_OPT_JUMP_K: -1 (default), 0 = off, 16..64; everything else RBG_EARG with the previous value in force"""
    L = ra.lib()
    assert capi.get_default_option(capi.OPT_JUMP_K) == -1
    for v in (-2, 1, 15, 65, 100):
        assert L.rbg_set_default_option(capi.OPT_JUMP_K, v) == -4, v
    for v in (0, 16, 44, 52, 60, 64, -1):
        assert L.rbg_set_default_option(capi.OPT_JUMP_K, v) == 0, v
        assert capi.get_default_option(capi.OPT_JUMP_K) == v


def test_jump_k_from_the_environment():
    code = "import sys; sys.path.insert(0, %r); from rowbowt_amd import capi; print(capi.get_default_option(capi.OPT_JUMP_K))" % ROOT
    def run(v):
        p = subprocess.run([__import__("sys").executable, "-c", code], env=dict(os.environ, RBG_JUMP_K=v), capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        return p.stdout.split()[-1], p.stderr
    assert run("44")[0] == "44" and run("0")[0] == "0"
    for bad in ("8", "65", "x"):
        out, err = run(bad)
        assert out == "-1" and "RBG_JUMP_K" in err and "ignored" in err
