"""GPU parity of rbg_marker_runs_plan_dev / rbg_marker_runs_fill_dev (rowbowt_amd/csrc/mk_build.hip) against tests/marker_build_model.py, exactly, at 4-byte
and at forced 8-byte positions, with the suffix array from capi.suffix_array.  The records, the scratch and the four outputs are regions of a guarded arena
(tests/arena.py): no byte outside the declared outputs changes and the inputs stay as they were.

The sweeps of mk_build.hip stride a grid capped at 2 048 workgroups of 256 lanes: CAP = 524 288 rows per pass (kMkGridCap * kMkThreads); a chunk is the 256
rows of one workgroup trip, a wave 64 of them."""
import functools
import os

import numpy as np
import pytest
import torch

import marker_build_cases as MC
import marker_build_model as MB
import rowbowt_amd as ra
from arena import Arena
from rowbowt_amd import capi
from sdsl_writer import decode_mab

pytestmark = pytest.mark.gpu
EARG = -4
CAP = 2048 * 256
ACGT = np.frombuffer(b"ACGT", np.uint8)
U64 = np.uint64
WIDTHS = [4, 8]


def _t(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


@functools.lru_cache(maxsize=None)
def sa_of(key):
    """the suffix array of a cached text, by the device build (held to tests/naive.py by tests/test_gpu_sa_build.py), once for both widths"""
    text = TEXTS[key]()
    return capi.suffix_array(torch.from_numpy(text).cuda()).cpu().numpy().astype(np.int64) & 0xFFFFFFFF


class Run:
    """one plan + fill on a guarded arena"""

    def __init__(self, sa, pb, pos, first, val, w, arena=None, stream=None):
        self.L = ra.lib()
        self.n, self.S, self.pb, self.w = len(sa), len(pos), pb, w
        self.nb = int(self.L.rbg_marker_runs_tmp_bytes(self.n, self.S, w, pb))
        cap = min(self.n, self.S * w)
        # (at most min(n, S w) rows are covered, so as many runs, 24 bytes each; every (row, record) pair gives one value at the most: S w)
        self.A = A = arena or Arena(self.n * pb + 24 * self.S + self.nb + 24 * cap + 8 * self.S * w + 16384, device="cuda")
        if arena is None:
            self.sa = A.carve_from("sa", np.asarray(sa).astype(np.uint32 if pb == 4 else np.uint64), align=pb)
            self.pos, self.first, self.val = (A.carve_from(k, np.asarray(a, U64), align=8) for k, a in (("pos", pos), ("first", first), ("val", val)))
            self.tmp = A.carve("tmp", self.nb, align=256)
            self.out = None
        self.st = stream if stream is not None else torch.cuda.current_stream().cuda_stream

    def plan(self, **kw):
        a = dict(sa=self.sa.ptr, n=self.n, pb=self.pb, pos=self.pos.ptr, first=self.first.ptr, val=self.val.ptr, S=self.S, w=self.w, tmp=self.tmp.ptr, nb=self.nb)
        a.update(kw)
        r, v = capi.U64(0xDEAD), capi.U64(0xBEEF)
        rc = self.L.rbg_marker_runs_plan_dev(a["sa"], a["n"], a["pb"], a["pos"], a["first"], a["val"], a["S"], a["w"], a["tmp"], a["nb"], capi.C.byref(r),
                                             capi.C.byref(v), self.st)
        return rc, int(r.value), int(v.value)

    def carve_out(self, nruns, nvals):
        A = self.A
        self.out = [A.carve("run_start", nruns * 8), A.carve("run_end", nruns * 8), A.carve("mk_off", (nruns + 1) * 8), A.carve("mk_vals", nvals * 8)]

    def fill(self, nruns, nvals, **kw):
        a = dict(sa=self.sa.ptr, n=self.n, pb=self.pb, pos=self.pos.ptr, first=self.first.ptr, val=self.val.ptr, S=self.S, w=self.w, tmp=self.tmp.ptr, nb=self.nb,
                 o0=self.out[0].ptr, o1=self.out[1].ptr, o2=self.out[2].ptr, o3=self.out[3].ptr)
        a.update(kw)
        return self.L.rbg_marker_runs_fill_dev(a["sa"], a["n"], a["pb"], a["pos"], a["first"], a["val"], a["S"], a["w"], a["tmp"], a["nb"], nruns, nvals, a["o0"],
                                               a["o1"], a["o2"], a["o3"], self.st)

    def results(self):
        return tuple(o.numpy(U64) for o in self.out)


def check(sa, pb, pos, first, val, w, want=None, tag=""):
    """plan and fill; the arrays equal the model's, the inputs are unchanged, no guard byte is written"""
    want = want if want is not None else MB.marker_runs(sa, pos, first, val)
    R = Run(sa, pb, pos, first, val, w)
    R.A.snapshot_all(["sa", "pos", "first", "val"])
    rc, nruns, nvals = R.plan()
    assert (rc, nruns, nvals) == (0, len(want[0]), len(want[3])), (tag, pb, w, rc, nruns, nvals, len(want[0]), len(want[3]))
    R.carve_out(nruns, nvals)
    assert R.fill(nruns, nvals) == 0, (tag, pb, w)
    torch.cuda.synchronize()
    R.A.check()
    R.A.assert_all_unchanged()
    for name, a, b in zip(("run_start", "run_end", "mk_off", "mk_vals"), R.results(), want):
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, (tag, pb, w, name, bad[:5], a[bad[:5]], b[bad[:5]])
    return R


# ---- 1. the reference's own array -----------------------------------------------------------------------------------------------------------------------
def _fixture_text():
    return MB.fixture_layout(10)["text"]


@pytest.mark.parametrize("pb", WIDTHS)
def test_fixture_pin(pb):
    F = MB.fixture_layout(10)
    _u, s, e, off, vals, wsize = decode_mab(open(os.path.join(MB.DATA, "small.fa.mab"), "rb").read())
    assert wsize == 10 and len(s) == 190
    check(sa_of("fixture"), pb, F["pos"], F["first"], F["val"], 10, want=tuple(a.astype(U64) for a in (s, e, off, vals)), tag="fixture")


# ---- 2. window edges -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pb", WIDTHS)
def test_window_edges(pb):
    text, sa = MC.edge_text(), sa_of("edges")
    for w in (1, 2, 10, 19, 64):
        pos, first, val = MC.edge_records(w)
        assert MB.records_ok(pos, first, len(text), w)
        want = MB.marker_runs(sa, pos, first, val)
        assert int(np.diff(want[2].astype(np.int64)).max()) == min(w, w + 3)      # rows with w values: the sort within a row
        assert int(pos[-1]) == len(text) - 2 and int(first.min()) == 0
        check(sa, pb, pos, first, val, w, want, tag="edges")


# ---- 3. the run rule -------------------------------------------------------------------------------------------------------------------------------------
def _copies_text(alternate):
    rng = np.random.default_rng(600)
    hap = rng.choice(ACGT, 40)
    alt = hap.copy()
    alt[20] = ACGT[(int(np.flatnonzero(ACGT == hap[20])[0]) + 1) % 4]
    return _t(b"#".join((alt if alternate and d % 2 else hap).tobytes() for d in range(600)) + b"\x01")


def copies_records(sites, w, alternate):
    docs = [(d * 41, [(o, MB.marker_value(1 if alternate and d % 2 and o == 20 else 0, 0, o)) for o in sites]) for d in range(600)]
    return MB.records(docs, w)


@pytest.mark.parametrize("pb", WIDTHS)
def test_run_rule(pb):
    for key, sites, alternate in (("copies", (20,), False), ("copies", (20, 23), False), ("copies alt", (20,), True)):
        sa = sa_of(key)
        pos, first, val = copies_records(sites, 10, alternate)
        want = MB.marker_runs(sa, pos, first, val)
        lens = (want[1] - want[0]).astype(np.int64) + 1
        if len(sites) == 1 and not alternate:
            # runs of 600 adjacent rows: they cross a wave, a workgroup and a chunk boundary
            assert (lens >= 600).any() and any(int(a) // 256 != int(b) // 256 for a, b in zip(want[0], want[1]))
        if len(sites) == 2:
            # adjacent rows with equal two-value lists stay runs of their own
            two = np.flatnonzero(np.diff(want[2].astype(np.int64)) == 2)
            assert len(two) >= 600 and (lens[two] == 1).all() and (np.diff(want[0][two].astype(np.int64)) == 1).any()
        if alternate:
            assert (lens == 300).any()
        check(sa, pb, pos, first, val, 10, want, tag=(key, sites))


# ---- 4. past one grid pass -------------------------------------------------------------------------------------------------------------------------------
SCALE_N = 2 * CAP + 1


def _scale_text():
    return np.append(np.random.default_rng(SCALE_N).choice(ACGT, SCALE_N - 1), 1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scale_records():
    """300 sites of one document, found from the suffix array: the suffixes of rows CAP - 1, CAP, CAP + 1, 2 CAP (the third pass's one row) and rows spread
    over both passes, thinned so that no two sites are closer than 12"""
    sa = sa_of("scale")
    rows = np.concatenate([[CAP - 1, CAP, CAP + 1, 2 * CAP], np.linspace(5, 2 * CAP - 5, 600).astype(np.int64)])
    sites = []
    for p in sa[rows].tolist():
        if p < SCALE_N - 1 and all(abs(p - q) >= 12 for q in sites):
            sites.append(p)
        if len(sites) == 300:
            break
    assert len(sites) == 300 and all(int(sa[r]) in sites for r in (CAP - 1, CAP, CAP + 1, 2 * CAP))
    return MB.records([(0, [(p, MB.marker_value(p % 2, 0, p)) for p in sorted(sites)])], 10)


@pytest.mark.parametrize("pb", WIDTHS)
def test_past_one_grid_pass(pb):
    sa = sa_of("scale")
    pos, first, val = scale_records()
    cov = MB.covered_rows(sa, pos, first)
    assert {CAP - 1, CAP, CAP + 1, 2 * CAP} <= set(cov.tolist()) and (cov < CAP).sum() > 100 and ((cov >= CAP) & (cov < 2 * CAP)).sum() > 100
    check(sa, pb, pos, first, val, 10, tag="scale")


# ---- 5. trivial sizes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pb", WIDTHS)
def test_trivial_sizes(pb):
    z = np.zeros(0, U64)
    one = np.zeros(1, U64)
    sa = sa_of("edges")
    R = check(sa, pb, z, z, z, 10, tag="S=0")                                                  # mk_off[0] = 0 only
    assert R.results()[2].tolist() == [0]
    check(sa, pb, np.array([5], U64), np.array([0], U64), np.array([MB.marker_value(3, 7, 5)], U64), 10, tag="S=1")
    check(np.zeros(1, np.int64), pb, one, one, np.array([9], U64), 1, tag="n=1")
    check(np.zeros(1, np.int64), pb, z, z, z, 64, tag="n=1 S=0")


def test_the_scratch_stays_below_n_plus_64_s_w():
    """the structural claim of DESIGN 6l: no array of n positions -- n / 8 + n / 32 bytes, 32 per row that can be covered, hipCUB's own and a header"""
    L = ra.lib()
    for n, S, w in ((2_000_000_501, 20_000_000, 10), (2_000_000_501, 1, 1), (1 << 20, 1000, 64), (30031, 30, 10), (1 << 36, 1 << 20, 64)):
        for pb in WIDTHS:
            if pb == 4 and n >= 0xFFFFFFF0:
                continue
            nb = int(L.rbg_marker_runs_tmp_bytes(n, S, w, pb))
            assert 0 < nb < n + 64 * S * w, (n, S, w, pb, nb)
            # (hipCUB's scans keep a few words per tile of at least a thousand items; the roundings to 256 are in the last term)
            assert nb <= 256 + n // 8 + n // 32 + 32 * min(n, S * w) + n // 1024 + (1 << 20), (n, S, w, pb, nb)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pb", WIDTHS)
def test_refusals_leave_the_outputs_untouched(pb):
    text, sa = MC.edge_text(), sa_of("edges")
    n = len(text)
    pos, first, val = MC.edge_records(10)
    R = Run(sa, pb, pos, first, val, 10)
    rc, nruns, nvals = R.plan()
    assert rc == 0 and nruns > 0
    R.carve_out(nruns, nvals)
    L = R.L
    assert L.rbg_marker_runs_tmp_bytes(0, 1, 10, pb) == 0 and L.rbg_marker_runs_tmp_bytes(n, 1, 0, pb) == 0 and L.rbg_marker_runs_tmp_bytes(n, 1, 65, pb) == 0
    assert L.rbg_marker_runs_tmp_bytes(n, n + 1, 10, pb) == 0 and L.rbg_marker_runs_tmp_bytes(1 << 33, 1, 10, 4) == 0 and L.rbg_marker_runs_tmp_bytes(n, 1, 10, 2) == 0
    bad = [dict(n=0), dict(w=0), dict(w=65), dict(sa=None), dict(pos=None), dict(first=None), dict(val=None), dict(tmp=None), dict(sa=R.sa.ptr + 1),
           dict(pos=R.pos.ptr + 4), dict(first=R.first.ptr + 4), dict(val=R.val.ptr + 4), dict(tmp=R.tmp.ptr + 8), dict(nb=R.nb - 1), dict(pb=2), dict(S=n + 1)]
    if pb == 4:
        bad.append(dict(n=1 << 33))
    for kw in bad:
        assert R.fill(nruns, nvals, **kw) == EARG, kw
    for kw in (dict(o0=None), dict(o1=None), dict(o2=None), dict(o3=None), dict(o0=R.out[0].ptr + 4), dict(o1=R.out[1].ptr + 4), dict(o2=R.out[2].ptr + 4),
               dict(o3=R.out[3].ptr + 4)):
        assert R.fill(nruns, nvals, **kw) == EARG, kw
    # counts that are not the plan's, and arguments that are not the plan's
    for a, b in ((nruns - 1, nvals), (nruns + 1, nvals), (nruns, nvals - 1), (nruns, nvals + 1), (0, 0)):
        assert R.fill(a, b) == EARG, (a, b)
    assert R.fill(nruns, nvals, w=11) == EARG and R.fill(nruns, nvals, S=R.S - 1) == EARG
    torch.cuda.synchronize()
    for o in R.out:
        R.A.check_untouched(o.name, [(0, o.nbytes)])
    R.A.check()
    # the plan: the same refusals, the counts untouched; then every way the records can break their rule
    for kw in bad:
        assert R.plan(**kw) == (EARG, 0xDEAD, 0xBEEF), kw
    assert R.L.rbg_marker_runs_plan_dev(R.sa.ptr, n, pb, R.pos.ptr, R.first.ptr, R.val.ptr, R.S, 10, R.tmp.ptr, R.nb, None, None, R.st) == EARG
    for what, (p, f) in {
        "pos not ascending": (np.array([5, 5], U64), np.array([0, 0], U64)),
        "pos descending": (np.array([9, 5], U64), np.array([0, 0], U64)),
        "first descending": (np.array([15, 20], U64), np.array([12, 11], U64)),
        "first past pos": (np.array([5], U64), np.array([6], U64)),
        "pos at n": (np.array([n], U64), np.array([n - 3], U64)),
        "window of w + 1": (np.array([30], U64), np.array([20], U64)),
    }.items():
        Q = Run(sa, pb, p, f, np.arange(len(p), dtype=U64), 10)
        assert Q.plan() == (EARG, 0xDEAD, 0xBEEF), what
        Q.carve_out(2, 2)
        assert Q.fill(2, 2) == EARG, what
        torch.cuda.synchronize()
        for o in Q.out:
            Q.A.check_untouched(o.name, [(0, o.nbytes)])
        Q.A.check()


# ---- 7. stream order -------------------------------------------------------------------------------------------------------------------------------------
def test_plan_and_fill_on_a_side_stream_behind_queued_work():
    sa = sa_of("edges")
    pos, first, val = MC.edge_records(10)
    want = MB.marker_runs(sa, pos, first, val)
    side = torch.cuda.Stream()
    R = Run(np.zeros(len(sa), np.int64), 4, np.zeros(len(pos), U64), np.zeros(len(pos), U64), np.zeros(len(pos), U64), 10, stream=side.cuda_stream)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        # the inputs arrive on the side stream, behind a stretch of queued work: a call that ran ahead of its stream would read zeros
        busy = torch.ones(1 << 22, device="cuda")
        for _ in range(20):
            busy = busy * 1.0001
        for reg, a in ((R.sa, sa.astype(np.uint32)), (R.pos, pos), (R.first, first), (R.val, val)):
            reg.u8.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda(), non_blocking=True)
        rc, nruns, nvals = R.plan()
        assert (rc, nruns, nvals) == (0, len(want[0]), len(want[3]))
        R.carve_out(nruns, nvals)
        assert R.fill(nruns, nvals) == 0
    side.synchronize()
    R.A.check()
    for a, b in zip(R.results(), want):
        assert (a == b).all()


# ---- 8. stale buffers ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pb", WIDTHS)
def test_a_small_input_after_a_large_one_in_the_same_buffers(pb):
    F = MB.fixture_layout(10)
    big = check(sa_of("fixture"), pb, F["pos"], F["first"], F["val"], 10, tag="large")
    sa = sa_of("edges")
    pos, first, val = MC.edge_records(2)
    want = MB.marker_runs(sa, pos, first, val)
    assert len(want[0]) < 190 and len(sa) < 30031
    # the same regions, not refilled: the small input lies at the front of the large one's
    for reg, a in ((big.sa, sa.astype(np.uint32 if pb == 4 else np.uint64)), (big.pos, pos), (big.first, first), (big.val, val)):
        raw = np.ascontiguousarray(a).view(np.uint8)
        reg.u8[:raw.size].copy_(torch.from_numpy(raw.copy()))
    small = Run(sa, pb, pos, first, val, 2, arena=big.A)
    small.sa, small.pos, small.first, small.val, small.tmp, small.out = big.sa, big.pos, big.first, big.val, big.tmp, big.out
    assert small.nb <= big.nb
    before = [o.numpy(U64) for o in big.out]
    rc, nruns, nvals = small.plan()
    assert (rc, nruns, nvals) == (0, len(want[0]), len(want[3]))
    assert small.fill(nruns, nvals) == 0
    torch.cuda.synchronize()
    big.A.check()
    for o, old, new, k in zip(big.out, before, want, (nruns, nruns, nruns + 1, nvals)):
        got = o.numpy(U64)
        assert (got[:k] == new).all() and (got[k:] == old[k:]).all(), o.name      # the small answer, and behind it what the large one left


TEXTS = {"fixture": _fixture_text, "edges": MC.edge_text, "copies": lambda: _copies_text(False), "copies alt": lambda: _copies_text(True), "scale": _scale_text}
