"""CPU checks of the completeness rule of the jump table (rbg_jump.h jump_complete_mask): which levels let an absent key end a read, on a host
model of the tables, and the field that reports them."""
import ctypes as C
import os
import subprocess

from rowbowt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jump_complete_rule(tmp_path):
    """tests/cpp/jump_complete_check.cpp under ASan + UBSan: all words inserted, one word skipped at either level (toeholds 0xFFFFFFF0, 0xFFFFFFFF,
    2^32, 2^64 - 2; 2^64 - 1 is expressible), no table, level 2 declined, a build that stopped early, the switch off -- the mask is the rule's, and
    no read whose word occurs in the text is ever ended at a probe"""
    exe = tmp_path / "jump_complete"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "jump_complete_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, timeout=300)
    assert p.returncode == 0 and b"jump complete ok" in p.stdout, p.stdout[-300:] + p.stderr[-300:]


def test_jump_info_complete_field_is_behind_level_2():
    """rbg_jump_info_t grew at its end once more: `complete` at byte 80, the 80 bytes before it where they were (capi.JumpInfo is that prefix)"""
    J, JC = capi.JumpInfo, capi.JumpInfoComplete
    assert [f[0] for f in JC._fields_[:-1]] == [f[0] for f in J._fields_] and JC._fields_[-1][0] == "complete"
    assert JC.complete.offset == C.sizeof(J) == 80 and C.sizeof(JC) == 88
    hdr = open(os.path.join(ROOT, "include", "rbg.h")).read()
    body = hdr[hdr.index("typedef struct rbg_jump_info_t"):hdr.index("} rbg_jump_info_t;")]
    assert body.rstrip().endswith("uint64_t complete;") and body.index("build2_ms") < body.index("uint64_t complete;")
    assert "RBG_JUMP_ABSENT_ENDS" in hdr
