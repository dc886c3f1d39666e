"""CPU-only checks of rb_markers' report calls (rbg_markers_report / rbg_markers_report_text and their device steps): the library exports
them, they refuse to run without a device, they check their parameters first, and the sort key the canon kernel relies on -- rotl64(m, 4) --
orders markers as marker_cmp does."""
import ctypes as C
import os

import numpy as np
import pytest

import rb_markers_model as RM
import rowbowt_amd as ra
from rowbowt_amd import capi

NEW = ("rbg_read_strands_bytes", "rbg_read_strands_dev", "rbg_marker_seeds_canon_tmp_bytes", "rbg_marker_seeds_canon_dev", "rbg_report_select_tmp_bytes",
       "rbg_report_select_dev", "rbg_markers_report", "rbg_markers_report_text")
ENODEV, EARG = -3, -4
M64 = 2**64 - 1


@pytest.fixture(scope="module")
def host(data_dir):
    rb = ra.load_rowbowt(os.path.join(data_dir, "small.fa"), ra.LoadRbwtFlag.MA, device=capi.DEVICE_NONE)
    yield rb
    rb.close()


def test_exports():
    L = ra.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert L.rbg_abi_version() == 3
    assert L.rbg_read_strands_bytes(0) == 16 and L.rbg_read_strands_bytes(8) == 32 and L.rbg_read_strands_bytes(9) == 48
    assert C.sizeof(capi.ReportParams) == 56 and capi.REPORT_SEED.itemsize == 48


def _code(fn, *a, **kw):
    with pytest.raises(ra.RbgError) as e:
        fn(*a, **kw)
    return e.value.code if hasattr(e.value, "code") else e.value.args[0]


def test_no_device_no_answer(host):
    seqs, off = ra.pack_reads([b"ACGTACGTAC", b"", b"nnAC"])
    names = [b"a", b"b", b"c"]
    for params in (capi.report_params(), capi.report_params(heuristic=True, best_strand=True, min_seed_len=5),
                   capi.report_params(lmem=True, ftab_k=4, wsize=8)):
        assert _code(host.markers_report, seqs, off, params) == ENODEV
        assert _code(host.markers_report_text, seqs, off, names, params) == ENODEV
    L, z = ra.lib(), np.zeros(8, np.uint64)
    p = capi.report_params()
    assert L.rbg_read_strands_dev(host.h, None, None, 0, 0, None, capi._p(z), None) == ENODEV
    assert L.rbg_marker_seeds_canon_dev(host.h, capi._p(z), 1, capi._p(z), 0, 0, 101, capi._p(z), 64, None) == ENODEV
    assert L.rbg_report_select_dev(host.h, None, None, None, 0, None, C.byref(p), capi._p(z), None, None, None, 0, None) == ENODEV


def test_argument_errors_come_first(host):
    seqs, off = ra.pack_reads([b"ACGTACGTAC"])
    # rowbowt.hpp:423-426: the ftab's k - 1 may not exceed wsize; :346-349: lmem seeding needs an ftab
    assert _code(host.markers_report, seqs, off, capi.report_params(wsize=4, ftab_k=6)) == EARG
    assert _code(host.markers_report_text, seqs, off, [b"r"], capi.report_params(wsize=4, ftab_k=6)) == EARG
    assert _code(host.markers_report, seqs, off, capi.report_params(lmem=True, ftab_k=0)) == EARG
    assert _code(host.markers_report_text, seqs, off, [b"r"], capi.report_params(lmem=True, ftab_k=0)) == EARG
    assert _code(host.markers_report, seqs, off, capi.report_params(wsize=5, ftab_k=6)) == ENODEV   # k - 1 == wsize is allowed
    bad = capi.report_params()
    bad.flags = 1 << 9
    assert _code(host.markers_report, seqs, off, bad) == EARG


def _rotl4(m):
    return ((m << 4) | (m >> 60)) & M64


def test_sort_key_is_marker_cmp():
    """sorted(set(mk), key=marker_key) == sort by rotl64(m, 4) + adjacent unique: the field layout (allele 60-63, seq 48-59, pos 0-47) makes
    marker_cmp's (seq, pos, allele) the numeric order of the rotated value"""
    rng = np.random.default_rng(5)

    def mk(seq, pos, allele):
        return (allele << 60) | (seq << 48) | pos

    edge = [0, mk(0xFFF, 2**48 - 1, 15), mk(0xFFF, 0, 0), mk(0, 2**48 - 1, 0), mk(0, 0, 15), mk(1, 0, 0), mk(0, 1, 0), mk(0, 0, 1)]
    vals = list(edge)
    for _ in range(3000):
        vals.append(mk(int(rng.integers(0, 4)) * 0x555, int(rng.integers(0, 6)) if rng.random() < 0.5 else int(rng.integers(0, 2**48)), int(rng.integers(0, 16))))
    vals += [int(v) for v in rng.choice(np.array(vals, dtype=np.uint64), 2000)]   # heavy duplication
    rng.shuffle(vals)
    want = sorted(set(vals), key=RM.marker_key)
    by_key = sorted(vals, key=_rotl4)
    got = [m for j, m in enumerate(by_key) if j == 0 or m != by_key[j - 1]]
    assert got == want
    assert len({_rotl4(m) for m in vals}) == len(set(vals))   # a bijection
    assert all((_rotl4(a) < _rotl4(b)) == (RM.marker_key(a) < RM.marker_key(b)) for a in edge for b in edge)
    assert all(_rotl4(m) >> 4 == (RM.get_seq(m) << 48 | (m & (2**48 - 1))) for m in vals)   # key >> 4 is (seq, pos)
