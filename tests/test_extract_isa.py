"""The compiled kernels of rowbowt_amd/csrc/extract.hip (tools/check_isa.py compiles the file to gfx950 assembly; no GPU needed): no scratch -- the walk keeps
its state in registers and the views are staged in LDS --, no 64-bit shift by the last allocated VGPR, and the instantiations the launchers are meant to
name: k_isa_rows and k_extract at both position widths."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extract_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_isa
    ks = [k for k in check_isa.scan(["extract.hip"], workers=1)["extract.hip"] if k[0].startswith("_ZN3rbg")]
    assert not check_isa.hazards(ks), check_isa.hazards(ks)
    assert sorted(k[0] for k in ks) == sorted(f"_ZN3rbg12_GLOBAL__N_1{name}I{p}EEvNS_6FlViewENS_7IsaViewE{rest}"
                                              for name, rest in (("10k_isa_rows", "PKmmPmPj"), ("9k_extract", "PKmPKjS5_mPhPjS9_")) for p in "jm")
    assert all(scratch == 0 for _n, _v, scratch, _s in ks), ks
