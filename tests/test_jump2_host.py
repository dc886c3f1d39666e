"""CPU checks of level 2 of the jump table (rbg_jump.h): the key {K2 symbols after the first K1, the parent range's lo} and the probe on a
host model of the table, and the option's range."""
import os
import subprocess

import rowbowt_amd as ra
from rowbowt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jump2_key_packing_and_probe(tmp_path):
    """tests/cpp/jump2_check.cpp under ASan + UBSan: the level-2 key from a staged-code model and from a text word for K2 in {16, 17, 31, 32, 33,
    47, 48} at parent lo 0, 1, 2^31, 2^32 - 1; masking from bit 2 K2 up; the probe against a linear scan on tables of 1, 2, 3 and 8 buckets;
    equal symbols under different parents are different keys"""
    exe = tmp_path / "jump2"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "jump2_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, timeout=300)
    assert p.returncode == 0 and b"jump2 ok" in p.stdout, p.stdout[-300:] + p.stderr[-300:]


def test_jump2_k_option_range():
    """RBG_OPT_JUMP2_K: -1 (default), 0 = off, 16..48; everything else RBG_EARG with the previous value in force"""
    L = ra.lib()
    assert capi.get_default_option(capi.OPT_JUMP2_K) == -1
    try:
        for v in (-2, 1, 15, 49, 64):
            assert L.rbg_set_default_option(capi.OPT_JUMP2_K, v) == -4, v
            assert capi.get_default_option(capi.OPT_JUMP2_K) == -1
        for v in (0, 16, 24, 40, 48, -1):
            assert L.rbg_set_default_option(capi.OPT_JUMP2_K, v) == 0, v
            assert capi.get_default_option(capi.OPT_JUMP2_K) == v
    finally:
        L.rbg_set_default_option(capi.OPT_JUMP2_K, -1)


def test_jump_info_struct_grew_at_its_end():
    """rbg_jump_info_t: the five fields of level 1 where they were (40 bytes, what rbg_jump_info writes), level 2 behind them"""
    import ctypes as C
    J = capi.JumpInfo
    assert [f[0] for f in J._fields_[:5]] == ["k", "keys", "bytes", "buckets", "build_ms"]
    assert J.k2.offset == 40 and C.sizeof(J) == 80
    hdr = open(os.path.join(ROOT, "include", "rbg.h")).read()
    assert "rbg_jump_info_sized" in hdr and "RBG_OPT_JUMP2_K = %d" % capi.OPT_JUMP2_K in hdr
