"""GPU parity of the marker directory at the bucket widths of a large index (rbg_mkdir.hpp; rbg_device.hpp marker_query; capi/upload_runs.ipp
upload_marker_table): marker tables whose (n, nruns) give the directory shifts 15, 16, 17 and 20 -- the widest buckets that still get 32-byte records, and the
4-byte directory alone beyond -- with runs that end and start on the last rows a record can name and runs of 65 535 and 65 536 values.  marker_query reads
nothing of the BWT but n, so the index is a synthetic run list of about 2^23 rows.  Against plain arithmetic on the arrays (the values of every run with
start <= hi && end >= lo, in run order); tests/cpp/mkrec_check.cpp pins the same (n, nruns) -> shift pairs against the header."""
import os

import numpy as np
import pytest

import rowbowt_amd as ra
from rowbowt_amd import capi
from gpu_common import _random_run_index, _with_layout

pytestmark = pytest.mark.gpu
N_ROWS = 8401260            # what the run list below sums to (mkrec_check.cpp: gpu_n)
BIG = 120                   # at shift 16: the runs of 65 535 and 65 536 values lie in buckets from here on, everything random below BIG - 2
# name -> (number of runs, the shift the rule gives for them)
CASES = {"s15": (200, 15), "s16": (100, 16), "s17": (40, 17), "s20": (7, 20), "s20cap": (3, 20)}


def _rule_shift(n, nruns):
    shift = 0
    while shift < 20 and (n >> shift) > 2 * nruns:
        shift += 1
    return shift


@pytest.fixture(scope="module")
def run_list():
    heads, lens, ssa, esa, n = _random_run_index(np.random.default_rng(61), 8000, 2098)
    assert n == N_ROWS
    return heads, lens, ssa, esa


def _load(run_list):
    with capi.default_option(capi.OPT_KMER_STEPS, 1):
        return _with_layout(capi.LAYOUT_RUNS, lambda: ra.RowBowt.from_runs(*run_list, device=0))


def _features(name, n):
    """(start, end, number of values) of the runs placed by hand, F = the first row of a bucket of W rows"""
    shift = CASES[name][1]
    W = 1 << shift
    if name == "s20cap":   # three runs: (n >> 20) = 8 > 2 * 3, the cap at 20 binds
        return [(W - 10, W, 2), (2 * W + 0x12345, 3 * W - 1, 1), (n - 300, n - 1, 3)]
    runs = [(W - 10, W, 2),                        # starts before F, ends on F
            (W + 1, W + 3, 1),                     # starts on F + 1
            (2 * W, 2 * W + 5, 3),                 # starts on F; three runs in this bucket
            (2 * W + 100, 3 * W - 2, 1),           # ends on the bucket's last row but one (F + 0xFFFE at shift 16)
            (3 * W - 1, 3 * W - 1, 2),             # starts and ends on its last row (F + 0xFFFF)
            (4 * W + 9, 5 * W, 4)]                 # ends on the next bucket's first row (F + 0x10000): clamped in the record
    runs.append((n - 300, n - 1, 1))               # ends on n - 1
    if name == "s20":                              # seven runs in eight buckets
        return runs[:1] + runs[2:] + [(6 * W + 0x10005, 7 * W + 1, 1)]
    runs += [(6 * W + 7, 7 * W - 1, 1),            # ends on the bucket's last row, from a wide run
             (8 * W + 50, 11 * W - 1, 2),          # ends on F + 0x2FFFF
             (12 * W, 15 * W - 1, 3),              # covers three whole buckets and nothing else
             (17 * W + 1, 17 * W + 1, 1), (17 * W + 3, 17 * W + 4, 2), (17 * W + 10, 17 * W + 20, 1), (18 * W - 16, 18 * W - 1, 1),   # four runs: overflow
             (19 * W + 5, 19 * W + 6, 0),          # no value
             (20 * W - 1, 20 * W + 2, 1)]          # starts on a bucket's last row and goes on
    if name == "s16":
        runs += [((BIG + 2) * W + 10, (BIG + 2) * W + 20, 65535),     # as many values as a record counts
                 ((BIG + 4) * W + 1, (BIG + 4) * W + 2, 1),
                 ((BIG + 4) * W + 100, (BIG + 4) * W + 200, 65536),   # one more: overflow, between two small runs of its bucket
                 ((BIG + 4) * W + 300, (BIG + 4) * W + 301, 2)]
    return sorted(runs)


_cases = {}


def _case(name):
    """the table, the queries and the model's answers of one case; built once, on the CPU alone, and never changed"""
    if name in _cases:
        return _cases[name]
    nruns, shift = CASES[name]
    n, W = N_ROWS, 1 << shift
    assert _rule_shift(n, nruns) == shift and (name != "s20cap" or (n >> 20) > 2 * nruns)
    rng = np.random.default_rng(shift * 100 + nruns)
    feats = sorted(_features(name, n))
    limit = (BIG - 2) * W if name == "s16" else n          # random runs and random queries stay below this row
    taken = sorted(feats)
    while len(taken) < nruns:                               # small runs wherever there is room, up to four to a bucket
        s = int(rng.integers(21 * W, limit - W))
        e = s + int(rng.choice([0, 0, 1, 4, W // 3]))
        if all(e < a or s > b for a, b, _ in taken):
            taken = sorted(taken + [(s, e, int(rng.integers(1, 10)))])
            for d in range(int(rng.integers(0, 4))):        # neighbours in the same bucket
                s2 = e + 2 + 3 * d
                if len(taken) < nruns and all(s2 < a or s2 > b for a, b, _ in taken):
                    taken = sorted(taken + [(s2, s2, 1)])
    starts = np.array([t[0] for t in taken], np.uint64)
    ends = np.array([t[1] for t in taken], np.uint64)
    off = np.concatenate([[0], np.cumsum([t[2] for t in taken])]).astype(np.uint64)
    assert len(starts) == nruns and (starts[1:] > ends[:-1]).all() and (ends >= starts).all() and int(ends[-1]) < n
    vals = rng.integers(0, 1 << 62, size=int(off[-1]), dtype=np.uint64)
    # queries: every hand-placed row and its neighbours as lo and as hi, at widths 0, 1, one bucket, two buckets - 1 / + 0 / + 1
    small = [t for t in feats if t[2] < 60000]
    rows = sorted({max(0, p + d) for t in small for p in t[:2] for d in (-1, 0, 1)} | {b * W + d for t in small for b in (t[0] // W, t[1] // W) for d in (0, W - 1)} |
                  {0, n - 1, n, n + 5})
    q = []
    for p in rows:
        for w in (0, 1, W - 1, W, 2 * W - 1, 2 * W, 2 * W + 1):
            q.append((p, p + w))
            if p >= w and p < limit:
                q.append((p - w, p))
    if name == "s16":
        q = [(lo, hi) for lo, hi in q if hi < BIG * W or lo >= n - 400]           # (none of these reaches the two large runs)
        for s, e, c in [t for t in feats if t[2] >= 60000]:                         # the few that do
            q += [(s, s), (e, e), (s - 1, s), (e, e + 1), (s - 1, s - 1), (e + 1, e + 1), (s + 1, e - 1), (s - W, s), (e, e + W), (s // W * W, s // W * W + W - 1),
                  (s // W * W - 1, s), (s - 2 * W - 1, s)]
        q.append(((BIG + 2) * W, (BIG + 5) * W - 1))                                # both at once
    lo_r = rng.integers(0, limit - 2 * W - 2, size=3000)
    w_r = np.where(rng.integers(0, 2, size=3000) == 0, rng.choice([0, 1, 5, W - 1, W, 2 * W + 1], size=3000), rng.integers(0, 2 * W, size=3000))
    lo = np.concatenate([np.array([a for a, _ in q], np.uint64), lo_r.astype(np.uint64)])
    hi = np.concatenate([np.array([b for _, b in q], np.uint64), (lo_r + w_r).astype(np.uint64)])
    assert (hi >= lo).all()
    # the model: first run with end >= lo, one past the last run with start <= hi (every run lies below n; a range from n on has none)
    f = np.searchsorted(ends, lo, side="left")
    l = np.searchsorted(starts, hi, side="right")
    l = np.where((l > f) & (lo < n), l, f)
    cnt = (off[l] - off[f]).astype(np.int64)
    # what keeps the comparison from being vacuous
    last_row = ((lo + np.uint64(1)) % np.uint64(W) == 0) | (((np.minimum(hi, np.uint64(n - 1)) + np.uint64(1)) % np.uint64(W) == 0))
    assert int(last_row.sum()) >= 20 and (cnt == 0).sum() >= 20 and (cnt > 0).sum() >= 500
    assert ((lo < n) & (hi >= n) & (cnt > 0)).any() and (lo >= n).sum() >= 10
    if name == "s16":
        assert (cnt == 65535).sum() >= 1 and (cnt >= 65536).sum() >= 1 and (cnt >= 60000).sum() <= 40
    assert int(cnt.sum()) * 8 < 40 << 20
    _cases[name] = dict(starts=starts, ends=ends, off=off, vals=vals, lo=lo, hi=hi, f=f, l=l, cnt=cnt)
    for a in _cases[name].values():
        a.setflags(write=False)
    return _cases[name]


def _expected(c, order=None):
    """the values of the queries, in the given order of the queries"""
    idx = np.arange(len(c["lo"])) if order is None else order
    return np.concatenate([c["vals"][int(c["off"][c["f"][i]]):int(c["off"][c["l"][i]])] for i in idx] + [c["vals"][:0]])


@pytest.mark.parametrize("name", list(CASES))
def test_sa_table(run_list, name, monkeypatch):
    """rb.markers_at(lo, hi) on the SA-row table, with the bucket records (where the gates allow them) and with RBG_MK_REC=0: both equal the model and each other"""
    c = _case(name)
    want_off = np.concatenate([[0], np.cumsum(c["cnt"])]).astype(np.uint64)
    want = _expected(c)
    got = {}
    for rec in ("1", "0"):
        monkeypatch.setenv("RBG_MK_REC", rec)
        rb = _load(run_list)       # (the SA table is immutable once attached: a fresh handle per table)
        try:
            rb.set_markers(c["starts"], c["ends"], c["off"], c["vals"])
            got[rec] = rb.markers_at(c["lo"], c["hi"])
        finally:
            rb.close()
        bad = np.nonzero(np.diff(got[rec][0].astype(np.int64)) != c["cnt"])[0]
        assert len(bad) == 0, (name, rec, [(int(c["lo"][i]), int(c["hi"][i])) for i in bad[:5]])
        assert (got[rec][0] == want_off).all() and (got[rec][1] == want).all(), (name, rec)
    assert (got["1"][0] == got["0"][0]).all() and (got["1"][1] == got["0"][1]).all()


@pytest.mark.parametrize("name", list(CASES))
def test_text_table(run_list, name, monkeypatch):
    """the text-position table through set_text_markers + markers_at_locs: l = lo, read length hi - lo + 1.  Queries of one length are the locations of one read, so
    the fill kernel's rounds of G locations run side by side with reads of a single location, also over the run of 65 536 values; group widths 4 and 64"""
    c = _case(name)
    length = (c["hi"] - c["lo"] + np.uint64(1)).astype(np.uint64)
    order = np.argsort(length, kind="stable")
    lens, per = np.unique(length[order], return_counts=True)
    assert per.max() > 64 and (per == 1).sum() > 100         # more than a round of the widest group; reads of one location
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    loc_off = np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
    locs = c["lo"][order]
    want = _expected(c, order)
    want_off = np.concatenate([[0], np.cumsum(c["cnt"][order])])[loc_off.astype(np.int64)].astype(np.uint64)
    rb = _load(run_list)
    try:
        for rec, groups in (("1", ("4", "64")), ("0", ("64",))):
            monkeypatch.setenv("RBG_MK_REC", rec)
            rb.set_text_markers(c["starts"], c["ends"], c["off"], c["vals"])
            for g in groups:
                monkeypatch.setenv("RBG_LOCMK_GROUP", g)
                mk_off, got = rb.markers_at_locs(locs, loc_off, off)
                assert (mk_off == want_off).all() and (got == want).all(), (name, rec, g)
    finally:
        rb.close()
