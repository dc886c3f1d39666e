"""CPU-only checks of the marker tally: its model (tests/tally_model.py) on the committed rb_markers goldens, the export order, and the
library's exports and argument checks without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import golden_values as G
import rb_markers_model as RM
import rowbowt_amd as ra
import tally_model as TM
from rowbowt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rbg_tally_create", "rbg_tally_free", "rbg_tally_reset", "rbg_tally_reserve", "rbg_tally_add_tmp_bytes", "rbg_tally_add_dev", "rbg_markers_tally",
       "rbg_tally_add_entries", "rbg_tally_export", "rbg_tally_info")
ENODEV, EARG = -3, -4


@pytest.mark.parametrize("name", ["toy_rb_markers_default.txt", "toy_rb_markers_heuristic.txt"])
def test_parser_on_goldens(name):
    text = open(os.path.join(ROOT, "tests", "golden", name)).read()
    table, entries = TM.tally_from_stdout(text)
    tokens = re.findall(r" (\d+)/(\d+)/(\d+)", text)
    assert tokens and sum(nf + nr for _, nf, nr, _ in entries) == len(tokens)             # the totals are the marker tokens of the text
    assert {TM.make_marker(int(s), int(p), int(a)) for s, p, a in tokens} == set(table)
    for m, nf, nr, ls in entries:                                                         # the fields come back as golden_values reads them
        tok = f"{RM.get_seq(m)}/{G.get_pos(m)}/{G.get_allele(m)}"
        lines = [ln for ln in text.splitlines() for t in ln.split(" ")[5:] if t == tok]
        assert nf == sum(ln.split(" ")[2] == "+" for ln in lines) and nr == sum(ln.split(" ")[2] == "-" for ln in lines)
        assert ls == sum(int(ln.split(" ")[4]) for ln in lines)
    assert TM.entries_from_tsv(TM.entries_tsv(entries)) == entries                        # the tool's file round-trips
    assert TM.tally_from_stdout("".join(ln + "\n" for ln in text.splitlines() if ln.endswith(" .")))[1] == []


def test_export_order():
    rng = np.random.default_rng(9)
    keys = [0, TM.M64, TM.make_marker(0xFFF, 0, 0), TM.make_marker(0, 2**48 - 1, 15), TM.make_marker(1, 5, 0), TM.make_marker(1, 5, 1)]
    keys += [TM.make_marker(int(rng.integers(0, 5)), int(rng.integers(0, 50)), int(rng.integers(0, 16))) for _ in range(400)]
    table = {m: (1, 2, 3) for m in keys}
    table[TM.make_marker(2, 2, 2)] = (0, 0, 7)                                           # no counts: not exported
    got = [e[0] for e in TM.sorted_entries(table)]
    assert got == sorted((m for m in table if m != TM.make_marker(2, 2, 2)), key=TM.rotl4)
    assert got == sorted(got, key=RM.marker_key) and got[0] == 0 and got[-1] == TM.M64    # (sequence, position, allele)


def test_exports_and_sizes():
    L = ra.lib()
    for name in NEW:
        assert hasattr(L, name) and name in capi.EXPORTS, name
    assert capi.TALLY_ENTRY.itemsize == 32
    assert L.rbg_tally_add_tmp_bytes(0) >= 256 and L.rbg_tally_add_tmp_bytes(1000) >= 8 * 1001


def test_no_device_no_tally(data_dir):
    rb = ra.load_rowbowt(os.path.join(data_dir, "small.fa"), ra.LoadRbwtFlag.MA, device=capi.DEVICE_NONE)
    L, h = ra.lib(), C.c_void_p()
    assert L.rbg_tally_create(rb.h, 0, C.byref(h)) == ENODEV and not h.value
    assert L.rbg_tally_create(rb.h, 0, None) == EARG
    seqs, off = ra.pack_reads([b"ACGTACGTAC"])
    p = capi.report_params()
    assert L.rbg_markers_tally(rb.h, capi._p(seqs), capi._p(off), 1, None, C.byref(p), None) == EARG
    z = np.zeros(8, np.uint64)
    assert L.rbg_tally_reset(None) == EARG and L.rbg_tally_reserve(None, 1) == EARG and L.rbg_tally_info(None, capi._p(z)) == EARG
    assert L.rbg_tally_add_entries(None, None, 0) == EARG and L.rbg_tally_export(None, None, None) == EARG
    assert L.rbg_tally_add_dev(None, None, 0, None, 0, None, 0, None) == EARG
    L.rbg_tally_free(None)
    rb.close()
