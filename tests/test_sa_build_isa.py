"""The compiled kernels of rowbowt_amd/csrc/sa_build.hip (tools/check_isa.py compiles the file to gfx950 assembly; no GPU needed): no kernel of namespace rbg
uses scratch, none takes a 64-bit shift amount from its last allocated VGPR, and the kernels the builder is made of are there at both position widths."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sa_build_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_isa
    ks = [k for k in check_isa.scan(["sa_build.hip"], workers=1)["sa_build.hip"] if k[0].startswith("_ZN3rbg")]
    assert not check_isa.hazards(ks), check_isa.hazards(ks)
    assert all(scratch == 0 for _n, _v, scratch, _s in ks), ks
    names = [k[0] for k in ks]
    for kern in ("k_sa_key0", "k_sa_flags0", "k_sa_rerank0", "k_sa_flags", "k_sa_rerank", "k_sa_compact", "k_sa_scatter", "k_bwt_flags", "k_bwt_fill"):
        for p in "jm":      # uint32_t, uint64_t
            assert any(f"{len(kern)}{kern}I{p}E" in n for n in names), (kern, p)
    for kern in ("k_sa_hist", "k_sa_keys", "k_sa_key_lo", "k_sa_key_hi"):
        assert sum(f"{len(kern)}{kern}" in n for n in names) == 1, kern
