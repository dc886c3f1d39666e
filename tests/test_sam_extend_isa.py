"""The ISA of sam_extend.hip (tools/check_isa.py cross-compiles it to gfx950 assembly, no GPU needed): tests/test_capi_host.py scans every k_*.hip against
tests/golden/kernel_set.json; this file is scanned here -- no 64-bit shift by the last allocated VGPR, no scratch (the walk keeps its state in registers and
writes its mismatches straight into its record), and the instantiations the launchers are meant to name, by name."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sam_extend_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_isa
    ks = check_isa.scan(["sam_extend.hip"], workers=1)["sam_extend.hip"]
    assert not check_isa.hazards(ks), check_isa.hazards(ks)
    mine = {n: (v, s) for n, v, s, _ in ks if n.startswith("_ZN3rbg")}
    assert all(s == 0 for _, s in mine.values()), {n: s for n, (_, s) in mine.items() if s}
    walks = sorted(n for n in mine if "k_extend_left" in n)
    # position width (j = uint32_t, m = uint64_t) x layout (Lb0 = slot tables, Lb1 = run-indexed)
    assert [n[n.index("k_extend_left"):][:21] for n in walks] == ["k_extend_leftIjLb0EEE", "k_extend_leftIjLb1EEE", "k_extend_leftImLb0EEE", "k_extend_leftImLb1EEE"], walks
    # what DESIGN.md 6i says of the walk's occupancy rests on these: two waves per SIMD on the slot layout (at most 256 VGPRs), three on the run-indexed one
    # (at most 168); today 198 and 129 / 143 (tools/check_isa.py prints them)
    assert all(mine[n][0] <= (256 if "Lb0" in n else 168) for n in walks), {n: mine[n][0] for n in walks}
    rest = sorted(n.split("_GLOBAL__N_1")[1][2:].split("ENS")[0] for n in mine if "k_extend_left" not in n)
    assert rest == ["k_sam_ext_items", "k_sam_len_ext", "k_sam_write_ext"], rest
