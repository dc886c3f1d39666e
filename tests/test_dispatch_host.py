"""CPU check of the launchers' width / flag dispatch (rowbowt_amd/csrc/rbg_dispatch.hpp), which is plain C++17 and compiles without HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_width_and_flags_reach_the_matching_instantiation(tmp_path):
    """tests/cpp/dispatch_check.cpp under ASan + UBSan: widths 4 and 8 with zero to three nested flags -- the lambda's tags carry exactly the
    type and constants the run-time facts name (static_assert inside, one counter per combination outside, each reached once); the `yes` / `no`
    tags carry their constants into a lambda called from an if / else-if chain; values, references and void pass through as the return value.
    (Which kernels the launchers themselves instantiate is tests/test_capi_host.py's comparison with tests/golden/kernel_set.json.)"""
    exe = tmp_path / "dispatch_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "dispatch_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, timeout=300)
    assert p.returncode == 0 and b"dispatch ok" in p.stdout, p.stdout[-300:] + p.stderr[-300:]
