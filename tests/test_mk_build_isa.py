"""The compiled kernels of rowbowt_amd/csrc/mk_build.hip (tools/check_isa.py compiles the file to gfx950 assembly; no GPU needed): no kernel of namespace rbg
uses scratch -- the sort of a row's values stays in registers at every width of the network --, none takes a 64-bit shift amount from its last allocated
VGPR, and the kernels the pass is made of are there, the sweeps at both position widths."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mk_build_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_isa
    ks = [k for k in check_isa.scan(["mk_build.hip"], workers=1)["mk_build.hip"] if k[0].startswith("_ZN3rbg")]
    assert not check_isa.hazards(ks), check_isa.hazards(ks)
    assert all(scratch == 0 for _n, _v, scratch, _s in ks), ks
    names = [k[0] for k in ks]
    for kern in ("k_mk_count", "k_mk_compact"):
        for p in "jm":      # uint32_t, uint64_t
            assert any(f"{len(kern)}{kern}I{p}E" in n for n in names), (kern, p)
    for kern in ("k_mk_cover", "k_mk_heads"):
        assert sum(f"{len(kern)}{kern}" in n for n in names) == 1, kern
    for w in (4, 16, 64):
        assert any(f"9k_mk_fillILi{w}EE" in n for n in names), w
