"""The numpy model of the marker build (tests/marker_build_model.py) against the two arrays that exist without it: the reference's own small.fa.mab, from
the layout its text has with windows of 10, and synth_pangenome.marker_array on two synthetic pangenomes.  No GPU."""
import os

import numpy as np
import torch

import marker_build_model as MB
import naive
from sdsl_writer import decode_mab
from rowbowt_amd.tools import synth_pangenome as SP

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def fixture_mab():
    _u, s, e, off, vals, wsize = decode_mab(open(os.path.join(DATA, "small.fa.mab"), "rb").read())
    return s.astype(np.uint64), e.astype(np.uint64), off.astype(np.uint64), vals.astype(np.uint64), wsize


def test_the_model_reproduces_the_reference_marker_array():
    F = MB.fixture_layout(10)
    assert len(F["text"]) == 30031 and len(F["pos"]) == 30
    # the 0|0 site is a record in all three documents, allele 0
    assert sorted(int(v) >> 60 for v in F["val"]).count(0) >= 10 + 1 + 1
    sa = naive.suffix_array(F["text"])
    assert MB.records_ok(F["pos"], F["first"], len(F["text"]), 10)
    got = MB.marker_runs(sa, F["pos"], F["first"], F["val"])
    s, e, off, vals, wsize = fixture_mab()
    assert wsize == 10 and len(s) == 190 and len(vals) == 190
    assert len(MB.covered_rows(sa, F["pos"], F["first"])) == 300
    for a, b in zip(got, (s, e, off, vals)):
        assert a.dtype == np.uint64 and (a == b).all()
    # no other window gives it
    for w in (9, 11):
        G = MB.fixture_layout(w)
        other = MB.marker_runs(sa, G["pos"], G["first"], G["val"])
        assert len(other[0]) != 190 or not (other[0] == s).all()
    shifted = MB.marker_runs(sa, F["pos"] + np.uint64(1), F["first"] + np.uint64(1), F["val"])
    assert len(shifted[0]) != 190 or not (shifted[0] == s).all()


def synth_records(text, info, w):
    """the site records synth_pangenome.marker_array infers from its text: a site is a column where some haplotype differs from the first"""
    unit, H, L = info["unit"], info["H"], info["L"]
    t = text.cpu().numpy()
    haps = t[:H * unit].reshape(H, unit)[:, :L]
    sites = np.flatnonzero((haps != haps[0][None, :]).any(axis=0))
    docs = [(h * unit, [(int(p), MB.marker_value(int(haps[h, p] != haps[0, p]), 0, int(p))) for p in sites]) for h in range(H)]
    return MB.records(docs, w)      # (marker_array clips a window where its haplotype starts: p >= 0 within the copy)


def test_the_model_equals_the_torch_marker_array():
    for L, H, rate in ((300, 6, 0.05), (60, 40, 0.2)):
        text, info = SP.make_text(L, H, rate, 7, "cpu")
        sa = SP.suffix_array(text)
        want = SP.marker_array(text, info, sa, 10)
        pos, first, val = synth_records(text, info, 10)
        assert MB.records_ok(pos, first, info["n"], 10)
        got = MB.marker_runs(sa.cpu().numpy(), pos, first, val)
        for a, b in zip(got, want):
            assert len(a) == len(b) and (a == b).all()
