"""GPU parity of the markers at located text positions (k_loc_markers.hip; rbg_set_text_markers, rbg_markers_at_locs, the plan / fill pair,
rbg_find_loc_markers_greedy_seeding, rb_locs) against the oracle: the locations from Oracle.greedy_locate on the index, the markers from
markers_at(l, (l + m - 1) mod 2^64) on a second Oracle that holds the text runs (tests/rb_locs_model.py)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import orc
import rowbowt_amd as ra
import sdsl_writer as W
from rowbowt_amd import capi
from gpu_common import ROOT, _with_layout, split
from rb_locs_model import expected_stdout, loc_markers, markers_at_loc
from test_rb_locs_model import mk, text_oracle

pytestmark = pytest.mark.gpu
M64 = 2**64 - 1
GROUPS = (4, 16, 64)
LAYOUTS_WIDTHS = [(capi.LAYOUT_SLOTS, 0), (capi.LAYOUT_RUNS, 0), (capi.LAYOUT_RUNS, 8)]


class forced_group:
    """RBG_LOCMK_GROUP for the calls inside (read at every launch); None: the width chosen on the device"""

    def __init__(self, g):
        self.g = g

    def __enter__(self):
        self.prev = os.environ.pop("RBG_LOCMK_GROUP", None)
        if self.g is not None:
            os.environ["RBG_LOCMK_GROUP"] = str(self.g)

    def __exit__(self, *exc):
        os.environ.pop("RBG_LOCMK_GROUP", None)
        if self.prev is not None:
            os.environ["RBG_LOCMK_GROUP"] = self.prev
        return False


def _load(S, layout=capi.LAYOUT_AUTO, pos_bytes=0):
    with capi.default_option(capi.OPT_POS_BYTES, pos_bytes):
        return _with_layout(layout, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))


def _grid_runs(n):
    """text runs every 40 positions, five long, with 1-3 values each: every window of 50 positions meets at least one"""
    runs = []
    for j, s in enumerate(range(3, n - 5, 40)):
        runs.append((s, s + 4, [mk(j % 7, s + t, (j + t) % 3) for t in range(1 + j % 3)]))
    return runs


def _arrays(runs):
    off = np.cumsum([0] + [len(r[2]) for r in runs]).astype(np.uint64)
    return (np.array([r[0] for r in runs], np.uint64), np.array([r[1] for r in runs], np.uint64), off,
            np.array([v for r in runs for v in r[2]], np.uint64))


def _want_at_locs(ot, locs, loc_off, off):
    """per read: the markers of its locations in order"""
    out = []
    for i in range(len(off) - 1):
        m = int(off[i + 1] - off[i])
        got = []
        for l in locs[int(loc_off[i]):int(loc_off[i + 1])]:
            got += markers_at_loc(ot, int(l), m)
        out.append(got)
    return out


def _dev_pair(rb, locs, loc_off, off, stream=None):
    """the _dev pair on caller-owned torch buffers (on `stream` if given): (rc of the plan, mk_off, mk)"""
    import torch
    dev = torch.device("cuda:0")
    N, L = len(off) - 1, ra.lib()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(dev)
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        d_locs = t(locs) if len(locs) else torch.zeros(1, dtype=torch.int64, device=dev)
        d_loc_off, d_off = t(loc_off), t(off)
        d_mk_off = torch.empty(N + 1, dtype=torch.int64, device=dev)
        tmp_bytes = int(L.rbg_loc_markers_tmp_bytes(N))
        d_tmp = torch.empty(max(tmp_bytes, 8), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        rc = L.rbg_loc_markers_plan_dev(rb.h, d_locs.data_ptr(), d_loc_off.data_ptr(), d_off.data_ptr(), N, d_mk_off.data_ptr(), d_tmp.data_ptr(),
                                        tmp_bytes, st)
        if rc:
            return rc, None, None
        mk_off = d_mk_off.cpu().numpy().view(np.uint64)
        d_mk = torch.empty(max(int(mk_off[N]), 1), dtype=torch.int64, device=dev)
        rc = L.rbg_loc_markers_fill_dev(rb.h, d_locs.data_ptr(), d_loc_off.data_ptr(), d_off.data_ptr(), N, d_mk_off.data_ptr(), d_mk.data_ptr(), st)
        assert rc == 0
        torch.cuda.current_stream().synchronize()
        return 0, mk_off, d_mk.cpu().numpy().view(np.uint64)[:int(mk_off[N])]


# ---- 1. parity over the read shapes every group width has to get right ---------------------------------------------------------------
@pytest.fixture(scope="module")
def shaped(synth):
    """reads of the synth index with their locations from the oracle (a stretch of the text occurs in up to eight haplotypes), of lengths 0, 1
    and 100, and -- the kernels see locations and lengths only -- lists of exactly 0, 1, G - 1, G, G + 1 and 3 G + 1 real locations for G in
    {4, 16, 64} under a read of length 100; the markers of all of them from the oracle"""
    S = synth
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    ot = text_oracle(_grid_runs(S.n))
    reads = S.sample_reads(150, 100, seed=3, sub_rate=0.3) + S.sample_reads(40, 60, seed=4, sub_rate=0.0, ragged=True)
    reads += [b"", b"A", b"N", S.text[:100].tobytes(), b"NN" + S.text[:60].tobytes(), S.text[S.n - 61:S.n - 1].tobytes() + b"NN"]
    per = [o.greedy_locate(q, 10)[0] for q in reads]
    pool = [l for q, ls in zip(reads, per) if len(q) == 100 for l in ls]
    want_counts = sorted({c for g in GROUPS for c in (0, 1, g - 1, g, g + 1, 3 * g + 1)})
    rng = np.random.default_rng(8)
    base = S.sample_reads(1, 100, seed=77, sub_rate=0.0)[0]
    for c in want_counts:               # lists of exactly c real locations under a read of length 100 (the kernel sees locations and lengths only)
        reads.append(base)
        per.append([int(x) for x in rng.choice(pool, size=c, replace=c > len(pool))])
    seqs, off = ra.pack_reads(reads)
    loc_off = np.cumsum([0] + [len(p) for p in per]).astype(np.uint64)
    locs = np.array([l for p in per for l in p], np.uint64)
    want = _want_at_locs(ot, locs, loc_off, off)
    # what keeps the comparison from being vacuous, on the oracle's output
    counts = np.diff(loc_off).astype(np.int64)
    lens = np.diff(off).astype(np.int64)
    assert len(reads) <= 300 and len(locs) <= 20000
    assert set(want_counts) <= set(counts.tolist()) and {0, 1, 100} <= set(lens.tolist())
    located = [i for i in range(len(reads)) if counts[i] > 0]
    assert 3 * sum(1 for i in located if want[i]) >= len(located)
    assert any(counts[i] > 64 and want[i] for i in range(len(reads)))
    yield S, o, ot, reads, seqs, off, locs, loc_off, want
    o.close()
    ot.close()


@pytest.mark.parametrize("group", [4, 16, 64, None])
def test_markers_at_locs_parity(shaped, group):
    """rbg_markers_at_locs and the plan / fill pair equal the oracle, once per forced group width and once with the width chosen on the device"""
    S, o, ot, reads, seqs, off, locs, loc_off, want = shaped
    rb = _load(S)
    try:
        rb.set_text_markers(*_arrays(_grid_runs(S.n)))
        with forced_group(group):
            mk_off, got = rb.markers_at_locs(locs, loc_off, off)
            assert split(mk_off, got) == want
            rc, d_off, d_mk = _dev_pair(rb, locs, loc_off, off)
            assert rc == 0 and (d_off == mk_off).all() and (d_mk == got).all()
            # a batch of one read, and an empty batch
            one_off, one = rb.markers_at_locs(locs[:int(loc_off[1])], loc_off[:2], off[:2])
            assert split(one_off, one) == want[:1]
            e_off, e = rb.markers_at_locs(np.zeros(0, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint64))
            assert e_off.tolist() == [0] and len(e) == 0
    finally:
        rb.close()


# ---- 2. table edges --------------------------------------------------------------------------------------------------------------------
def _edge_tables(n):
    big = [mk(1, t, t % 3) for t in range(150)]                      # more values than one fill round of any width copies
    return {
        "overflow": [(100 + 2 * j, 100 + 2 * j, [mk(0, j, 1)]) for j in range(12)] + [(900, 905, [mk(0, 900, 0)])],   # a bucket with more than three runs
        "spanning": [(50, 20050, [mk(0, 50, 1), mk(0, 51, 2)]), (20060, 20061, [mk(0, 20060, 1)]), (n - 9, n - 1, [mk(2, 5, 1)])],   # a run over several buckets; one ending at n - 1
        "big": [(10, 12, [mk(0, 10, 1)]), (300, 340, big), (500, 501, [mk(0, 500, 2)])],
        "one": [(n // 2, n // 2 + 3, [mk(0, 1, 1), mk(0, 2, 0)])],
        "none": [],
    }


@pytest.mark.parametrize("name", ["overflow", "spanning", "big", "one", "none"])
def test_table_edges(synth, name, monkeypatch):
    """against the oracle, and with RBG_MK_REC=0 (directory + arrays) against the same"""
    S = synth
    n = S.n
    runs = _edge_tables(n)[name]
    ot = text_oracle(runs) if runs else None
    rng = np.random.default_rng(5)
    # locations around every run's ends, at the text's ends, random ones; lengths 1, 7, 100 and 3000 (lo and hi in different buckets)
    pts = sorted({max(0, min(n - 1, p + d)) for r in runs for p in (r[0], r[1]) for d in (-101, -7, -1, 0, 1, 7)} | {0, 1, n - 2, n - 1, n - 100} |
                 set(int(x) for x in rng.integers(0, n, 40)))
    lens = [1, 7, 100, 3000]
    off = np.cumsum([0] + lens).astype(np.uint64)
    loc_off = (np.arange(len(lens) + 1) * len(pts)).astype(np.uint64)
    locs = np.array(pts * len(lens), np.uint64)
    want = _want_at_locs(ot, locs, loc_off, off) if ot else [[] for _ in lens]
    if ot:
        assert any(want)
        ot.close()
    got = []
    for rec in ("1", "0"):
        monkeypatch.setenv("RBG_MK_REC", rec)
        rb = _load(S)
        try:
            rb.set_text_markers(*_arrays(runs))
            for g in (4, 64):
                with forced_group(g):
                    mk_off, vals = rb.markers_at_locs(locs, loc_off, off)
                    assert split(mk_off, vals) == want, (rec, g)
            got.append((mk_off.tolist(), vals.tolist()))
        finally:
            rb.close()
    assert got[0] == got[1]


# ---- 3. location edges through the real path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,pos_bytes", LAYOUTS_WIDTHS)
def test_location_edges_real_path(synth, layout, pos_bytes):
    """rbg_find_loc_markers_greedy_seeding: a read that extends text[:k] to the left (its location wraps below zero), a read overhanging the end of
    the text, max_hits 1 and 3 and unbounded; on both layouts and position widths"""
    S = synth
    n = S.n
    rb = _load(S, layout, pos_bytes)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    runs = [(0, 30, [mk(0, 0, 1)])] + [r for r in _grid_runs(n) if r[0] > 40 and r[1] < n - 20] + [(n - 6, n - 1, [mk(3, 9, 2), mk(3, 10, 0)])]
    ot = text_oracle(runs)
    try:
        assert rb.info().pos_bytes == (pos_bytes or 4)
        rb.set_text_markers(*_arrays(runs))
        reads = [b"NNN" + S.text[:45].tobytes(), S.text[n - 41:n - 1].tobytes() + b"NNN", b"", b"ACG"]
        reads += S.sample_reads(60, 100, seed=21, sub_rate=0.3) + S.sample_reads(20, 50, seed=22, sub_rate=0.0, ragged=True)
        seqs, off = ra.pack_reads(reads)
        wrapped = o.greedy_locate(reads[0], 10)[0]
        assert M64 - 2 in wrapped and (n - 41) in o.greedy_locate(reads[1], 10)[0]
        for max_hits in (M64, 1, 3):
            loc_off, locs, mk_off, got = rb.find_loc_markers_greedy_seeding(seqs, off, 10, max_hits)
            wl = [loc_markers(o, ot, q, 10, max_hits) for q in reads]
            assert split(loc_off, locs) == [w[0] for w in wl], max_hits
            assert split(mk_off, got) == [w[1] for w in wl], max_hits
        full = [loc_markers(o, ot, q, 10)[1] for q in reads]
        assert mk(3, 9, 2) in full[1] and sum(1 for w in full if w) >= 40
        # a batch without any location
        loc_off, locs, mk_off, got = rb.find_loc_markers_greedy_seeding(*ra.pack_reads([b"NNNN", b""]), 10)
        assert loc_off.tolist() == [0, 0, 0] and mk_off.tolist() == [0, 0, 0] and len(locs) == 0 and len(got) == 0
    finally:
        rb.close()
        o.close()
        ot.close()


# ---- 4. contract ---------------------------------------------------------------------------------------------------------------------
def test_contract(shaped):
    import torch
    S, o, ot, reads, seqs, off, locs, loc_off, want = shaped
    rb = _load(S)
    L = ra.lib()
    try:
        # no table: RBG_ENOTLOADED from every call
        for call in (lambda: rb.markers_at_locs(locs, loc_off, off), lambda: rb.find_loc_markers_greedy_seeding(seqs, off, 10)):
            with pytest.raises(capi.RbgError) as ei:
                call()
            assert ei.value.code == -6
        assert _dev_pair(rb, locs, loc_off, off)[0] == -6
        assert L.rbg_loc_markers_fill_dev(rb.h, None, None, None, 0, None, None, None) == -6
        # RBG_EARG: unsorted runs, overlapping runs, a run at or beyond n
        for s, e in (([50, 10], [55, 15]), ([10, 14], [14, 20]), ([10], [S.n]), ([S.n], [S.n + 3])):
            with pytest.raises(capi.RbgError) as ei:
                rb.set_text_markers(s, e, np.arange(len(s) + 1, dtype=np.uint64), np.arange(len(s), dtype=np.uint64))
            assert ei.value.code == -4, (s, e)
        # setting the table twice leaves hbm_bytes where one setting does; the second table answers
        base = int(rb.info().hbm_bytes)
        arrays = _arrays(_grid_runs(S.n))
        rb.set_text_markers([7], [9], [0, 1], [mk(0, 7, 1)])
        rb.set_text_markers(*arrays)
        once = int(rb.info().hbm_bytes)
        rb.set_text_markers(*arrays)
        assert int(rb.info().hbm_bytes) == once and once > base
        mk_off, got = rb.markers_at_locs(locs, loc_off, off)
        assert split(mk_off, got) == want
        # the SA-row table is untouched by it: none was set
        assert not rb.info().has_markers
        # a replica on the same device answers like the primary; it refuses a table of its own
        rep = rb.replicate(0)
        try:
            r_off, r_got = rep.markers_at_locs(locs, loc_off, off)
            assert (r_off == mk_off).all() and (r_got == got).all()
            with pytest.raises(capi.RbgError):
                rep.set_text_markers(*arrays)
        finally:
            rep.close()
        # the _dev pair on a non-default stream with caller-owned buffers equals the host call
        rc, d_off, d_mk = _dev_pair(rb, locs, loc_off, off, stream=torch.cuda.Stream())
        assert rc == 0 and (d_off == mk_off).all() and (d_mk == got).all()
    finally:
        rb.close()


# ---- 5. rb_locs ------------------------------------------------------------------------------------------------------------------------
def _run_rb_locs(args):
    exe = os.path.join(ROOT, "rowbowt_amd", "rb_locs")
    p = subprocess.run([exe] + args, capture_output=True, timeout=120)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.fixture(scope="module")
def toy_files(synth, tmp_path_factory):
    """the synth index as the reference's files: .rbwt, .tsa, .docs, and the text runs as .midx (written with the .mab writer)"""
    S = synth
    d = tmp_path_factory.mktemp("rb_locs")
    prefix = str(d / "toy")
    with open(prefix + ".rbwt", "wb") as f:
        f.write(W.rbwt_bytes(S.heads, S.lens.astype(np.int64), 2))
    with open(prefix + ".tsa", "wb") as f:
        f.write(W.tsa_bytes(S.n, *W.tsa_arrays_from_samples(S.n, S.ssa, S.esa)))
    with open(prefix + ".docs", "w") as f:
        f.write("".join(f"{nm} {st}\n" for nm, st in zip(S.doc_names, S.doc_starts)))
    runs = _grid_runs(S.n)
    s, e, off, vals = _arrays(runs)
    with open(prefix + ".midx", "wb") as f:
        f.write(W.mab_bytes(s, e, off, vals, 10, universe=S.n))
    return prefix, runs


def test_rb_locs_stdout(synth, toy_files, tmp_path):
    """stdout equals the model's byte for byte, plain and gzip input, with -w 5 -m 2 and with the defaults; a missing .midx exits 1"""
    S = synth
    prefix, runs = toy_files
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    ot = text_oracle(runs)
    try:
        reads = S.sample_reads(40, 100, seed=31, sub_rate=0.3) + [b"NNN" + S.text[:45].tobytes(), S.text[S.n - 41:S.n - 1].tobytes() + b"NN", b"ACGTA", b"acgtacgtacgtacgt"]
        records = [(b"read%d" % i, q) for i, q in enumerate(reads)]
        blob = b"".join(b"@" + nm + b" a description\n" + q + b"\n+\n" + b"~" * len(q) + b"\n" for nm, q in records)
        plain, gz = tmp_path / "q.fq", tmp_path / "q.fq.gz"
        plain.write_bytes(blob)
        with gzip.open(gz, "wb") as f:
            f.write(blob)
        want_default = expected_stdout(o, ot, records)
        want_w5m2 = expected_stdout(o, ot, records, wsize=5, max_hits=2)
        assert want_default.count("/") > 100 and want_default != want_w5m2
        for path in (plain, gz):
            rc, out, err = _run_rb_locs([prefix, str(path)])
            assert rc == 0, err
            assert out == want_default
            rc, out, err = _run_rb_locs(["-w", "5", "-m", "2", "-o", str(tmp_path / "unused"), prefix, str(path)])
            assert rc == 0, err
            assert out == want_w5m2
        os.rename(prefix + ".midx", prefix + ".midx.away")
        try:
            rc, out, err = _run_rb_locs([prefix, str(plain)])
            assert rc == 1 and out == "" and ".midx" in err
        finally:
            os.rename(prefix + ".midx.away", prefix + ".midx")
    finally:
        o.close()
        ot.close()


def test_cpp_shim_loc_markers(synth, toy_files, tmp_path):
    """rowbowt_gpu.hpp: load_text_markers + find_loc_markers_greedy_seeding_batch print what the C-ABI call returns, and that is the model's"""
    S = synth
    prefix, runs = toy_files
    exe = tmp_path / "loc_markers_shim_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rowbowt_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "loc_markers_shim_check.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "rowbowt_amd"), "-lrbg", "-Wl,-rpath," + os.path.join(ROOT, "rowbowt_amd")])
    reads = S.sample_reads(12, 80, seed=33, sub_rate=0.3) + [b"NNN" + S.text[:45].tobytes(), b"ACG"]
    qfile = tmp_path / "q.txt"
    qfile.write_bytes(b"\n".join(reads) + b"\n")
    p = subprocess.run([str(exe), prefix, str(qfile), "10", "3"], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    ot = text_oracle(runs)
    try:
        want = []
        for q in reads:
            locs, mks = loc_markers(o, ot, q, 10, 3)
            want.append("locs" + "".join(f" {l}" for l in locs))
            want.append("mk" + "".join(f" {m}" for m in mks))
        want.append("same 1")
        assert p.stdout.decode().splitlines() == want
    finally:
        o.close()
        ot.close()
