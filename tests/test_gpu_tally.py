"""The marker tally on the GPU (k_tally.hip; rbg_tally_*, rbg_markers_tally, rb_markers --tally) against the model: the tally of the lines
rb_markers would print (tests/tally_model.py over tests/rb_markers_model.py::expected_stdout), exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orc
import rb_markers_model as RM
import rowbowt_amd as ra
import tally_model as TM
from gpu_common import _run_rb_markers
from lmem_model import LmemAsGreedy
from rowbowt_amd import capi
from synth import SynthIndex

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2**64 - 1
EARG = -4


@pytest.fixture(scope="module")
def toy_reads(data_dir):
    """the read set of the report tests: the two toy FASTQ files, 300 sampled reads of both strands with substitutions, a short and an empty read"""
    text = open(os.path.join(data_dir, "small.fa"), "rb").read().split(b"\n", 1)[1].replace(b"\n", b"")
    rng = np.random.default_rng(77)
    recs = []
    for fn in ("simple_query.fq", "error_query.fq"):
        names, seqs = orc.read_fastx(os.path.join(data_dir, fn))
        recs += list(zip(names, seqs))
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    for i in range(300):
        p = int(rng.integers(0, len(text) - 101))
        q = bytearray(text[p:p + 101])
        if i % 2:
            q = bytearray(bytes(q).translate(comp)[::-1])
        for _ in range(int(rng.integers(0, 3))):
            q[int(rng.integers(0, 101))] = b"ACGTN"[int(rng.integers(0, 5))]
        if i % 7 == 0:
            q = bytearray(bytes(q).lower())
        recs.append((f"syn{i}".encode(), bytes(q)))
    recs.append((b"short", b"ACG"))
    recs.append((b"empty", b""))
    return recs


def _coins(n):
    b = RM.Booler()
    return np.array([1 if b.get_bool() else 0 for _ in range(n)], dtype=np.uint8)


def _entries(t):
    e = t.export()
    return [(int(x["marker"]), int(x["n_fwd"]), int(x["n_rev"]), int(x["len_sum"])) for x in e]


def _feed(rb, t, recs, coins=None, **kw):
    seqs, off = ra.pack_reads([s for _, s in recs])
    if coins is None and kw.get("heuristic"):
        coins = _coins(len(recs))
    rb.markers_tally(seqs, off, capi.report_params(**kw), coins, t)


def _tally(rb, recs, hint=0, **kw):
    t = capi.Tally(rb, hint)
    _feed(rb, t, recs, **kw)
    got, info = _entries(t), t.info()
    t.close()
    assert info["dropped"] == 0 and 2 * info["entries"] <= info["capacity"] and info["entries"] == len(got)
    return got


def _want(o, recs, **kw):
    return TM.tally_from_stdout(RM.expected_stdout(o, recs, **kw))[1]


PARAM_SETS = [dict(), dict(wsize=10, max_range=3, min_range=2), dict(wsize=5), dict(heuristic=True),
              dict(heuristic=True, best_strand=True, min_seed_len=30, read_len=101),
              dict(heuristic=True, min_seed_len=25, clear_conflicting=True, clear_identical=True, read_len=50, wsize=8)]


@pytest.fixture(scope="module")
def want_default(small, toy_reads):
    return _want(small[1], toy_reads)


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", PARAM_SETS, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()) or "default")
def test_tally_toy(small, toy_reads, kw):
    rb, o = small
    want = _want(o, toy_reads, **kw)
    assert _tally(rb, toy_reads, **kw) == want
    if not kw:
        assert want and any(nf and nr for _, nf, nr, _ in want)   # markers seen on lines of both strands


def test_tally_ftab_and_lmem(small, toy_reads):
    rb, o = small
    long_recs = [r for r in toy_reads if len(r[1]) >= 6]
    for kw in (dict(wsize=8, ftab_k=6), dict(heuristic=True, best_strand=True, min_seed_len=20, ftab_k=6)):
        assert _tally(rb, long_recs, **kw) == _want(o, long_recs, **kw)
    dozen = toy_reads[:4] + toy_reads[40:46] + toy_reads[-2:]
    lm = LmemAsGreedy(o)
    for kw in (dict(wsize=8, ftab_k=6), dict(wsize=8, ftab_k=6, heuristic=True, best_strand=True, min_seed_len=30)):
        want = _want(lm, dozen, **kw)
        assert _tally(rb, dozen, lmem=True, **kw) == want and want


# ---- 2. accumulation -------------------------------------------------------------------------------------------------------------------

def test_tally_accumulates(small, toy_reads, want_default, monkeypatch):
    rb, o = small
    before = rb.info().hbm_bytes
    t = capi.Tally(rb, 0)
    assert rb.info().hbm_bytes == before + 64 * 32 + 64            # the handle's allocations are the index's
    half = len(toy_reads) // 2
    _feed(rb, t, toy_reads[:half])
    _feed(rb, t, toy_reads[half:])
    assert _entries(t) == want_default
    info = t.info()
    assert info["records"] == len(RM.expected_stdout(o, toy_reads).splitlines()) and info["elements"] == sum(nf + nr for _, nf, nr, _ in want_default)
    t.reset()
    after = t.info()
    assert _entries(t) == [] and after["capacity"] == info["capacity"] and after["entries"] == after["records"] == after["elements"] == 0
    for chunk in ("150", "1"):                                      # many passes (a pass holds at least one read)
        monkeypatch.setenv("RBG_REPORT_CHUNK", chunk)
        _feed(rb, t, toy_reads)
        assert _entries(t) == want_default, chunk
        t.reset()
    monkeypatch.delenv("RBG_REPORT_CHUNK")
    _feed(rb, t, [])                                                # N = 0
    assert _entries(t) == [] and t.info()["records"] == 0
    kw = dict(heuristic=True, best_strand=True, min_seed_len=30)    # the coins split with the reads
    coins = _coins(len(toy_reads))
    _feed(rb, t, toy_reads[:half], coins=coins[:half], **kw)
    _feed(rb, t, toy_reads[half:], coins=coins[half:], **kw)
    assert _entries(t) == _want(o, toy_reads, **kw)
    t.close()
    assert rb.info().hbm_bytes == before


def test_tally_without_markers():
    S = SynthIndex(L=1500, H=5, n_sites=30, seed=23)
    rb = ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0)
    reads = [(f"n{i}".encode(), q) for i, q in enumerate(S.sample_reads(40, 30, seed=7, sub_rate=0.1) + [b"ACNNGT", b""])]
    t = capi.Tally(rb, 0)
    _feed(rb, t, reads, wsize=4)
    info = t.info()
    assert _entries(t) == [] and info["entries"] == 0 and info["elements"] == 0 and info["records"] > 0 and info["capacity"] == 64
    t.close()
    rb.close()


# ---- 3. growth -------------------------------------------------------------------------------------------------------------------------

def test_tally_grows():
    """the dense synthetic marker table of the report tests (300 positions x 3 sequences x 4 alleles of keys, records of thousands of markers) into a
    tally that starts at 64 slots: a first grow for 40 merged entries, a second one -- which re-inserts those 40 -- for the reads"""
    rng = np.random.default_rng(19)
    S = SynthIndex(L=1500, H=5, n_sites=30, seed=23)
    n = int(np.sum(S.lens))
    rb = ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    nruns = n // 3
    starts = np.arange(nruns, dtype=np.uint64) * np.uint64(3)
    ends = starts + np.uint64(2)
    per = rng.integers(0, 200, nruns)
    off = np.concatenate(([0], np.cumsum(per))).astype(np.uint64)
    vals = (rng.integers(0, 300, int(off[-1]), dtype=np.uint64) | (rng.integers(0, 3, int(off[-1])).astype(np.uint64) << np.uint64(48))
            | (rng.integers(0, 4, int(off[-1])).astype(np.uint64) << np.uint64(60)))
    rb.set_markers(starts, ends, off, vals)
    o.set_markers(starts, ends, off, vals)
    reads = [(f"d{i}".encode(), q) for i, q in enumerate(S.sample_reads(6, 40, seed=5, sub_rate=0.1) + [b"ACGTTGCA", b"C"])]
    kw = dict(wsize=1, max_range=M64)
    table, want = TM.tally_from_stdout(RM.expected_stdout(o, reads, **kw))
    assert len(want) > 1000 and max(nf + nr for _, nf, nr, _ in want) > 4
    t = capi.Tally(rb, 0)
    assert t.info()["capacity"] == 64
    first = np.zeros(40, capi.TALLY_ENTRY)
    first["marker"] = [TM.make_marker(7, j, j % 16) for j in range(20)] + [m for m, _, _, _ in want[:20]]    # 20 keys of their own, 20 the reads will hit
    first["n_fwd"], first["n_rev"], first["len_sum"] = np.arange(40) % 3, 1, np.arange(40) * 1000
    t.add_entries(first)
    assert t.info()["grows"] == 1 and t.info()["capacity"] == 128
    _feed(rb, t, reads, **kw)
    info = t.info()
    both = TM.add_tables(table, {int(e["marker"]): (int(e["n_fwd"]), int(e["n_rev"]), int(e["len_sum"])) for e in first})
    assert _entries(t) == TM.sorted_entries(both)
    assert info["grows"] >= 2 and info["dropped"] == 0 and 2 * info["entries"] <= info["capacity"] and info["entries"] == len(both)
    t.close()
    rb.close()
    o.close()


# ---- 4. contention and combining -------------------------------------------------------------------------------------------------------

def test_tally_contention_and_combining(small, toy_reads, want_default, monkeypatch):
    rb, o = small
    one = next(r for r in toy_reads if _want(o, [r]))
    single = _want(o, [one])
    want = [(m, 512 * nf, 512 * nr, 512 * ls) for m, nf, nr, ls in single]
    results = []
    for combine in (None, "0", "1"):
        if combine is None:
            monkeypatch.delenv("RBG_TALLY_COMBINE", raising=False)
        else:
            monkeypatch.setenv("RBG_TALLY_COMBINE", combine)
        assert _tally(rb, [one] * 512) == want, combine
        results.append(_tally(rb, toy_reads))
        shuffled = [toy_reads[i] for i in np.random.default_rng(4).permutation(len(toy_reads))]
        results.append(_tally(rb, shuffled))
    assert all(r == want_default for r in results)


# ---- 5. rbg_tally_add_dev on hand-made records -----------------------------------------------------------------------------------------

def test_tally_add_dev_direct(small):
    import torch
    rb, _ = small
    rng = np.random.default_rng(41)
    a0, a1 = TM.make_marker(3, 1000, 0), TM.make_marker(3, 1000, 1)          # two keys that differ only in the allele bits
    pool = [TM.make_marker(int(rng.integers(0, 4)), int(rng.integers(0, 2**40)), int(rng.integers(0, 16))) for _ in range(40)]
    segs = [([0, M64, a0, a1], 0, 20), ([], 1, 7), ([a0, M64, 0], 1, 33), ([a1], 0, 2**63), ([a1], 1, 2**63 + 5),   # (len_sum wraps)
            ([pool[int(j)] for j in rng.integers(0, 40, 5000)], 0, 11), ([], 0, 0), ([pool[3], pool[3], 0], 1, 9)]
    gap = 2
    flat, recs, at = [], np.zeros(len(segs), capi.REPORT_SEED), 0
    for r, (s, strand, qlen) in enumerate(segs):
        flat += [0xDEAD0000 + at] * gap                                        # words between the segments: no record points at them
        at += gap
        recs[r] = (5, 1, qlen, at, at + len(s), strand, 0)
        flat += s
        at += len(s)
    want = {}
    for s, strand, qlen in segs:
        for m in s:
            nf, nr, ls = want.get(m, (0, 0, 0))
            want[m] = (nf + (strand == 0), nr + (strand == 1), (ls + qlen) & M64)
    R, M = len(segs), sum(len(s) for s, _, _ in segs)
    d_recs = torch.from_numpy(recs.view(np.uint8).copy()).to("cuda:0")
    d_mk = torch.from_numpy(np.array(flat, dtype=np.uint64).view(np.int64)).to("cuda:0")
    L = ra.lib()
    tmp_bytes = L.rbg_tally_add_tmp_bytes(R)
    d_tmp = torch.zeros(tmp_bytes, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    t = capi.Tally(rb, 0)
    info0 = t.info()
    assert L.rbg_tally_add_dev(t.h, d_recs.data_ptr(), R, d_mk.data_ptr(), M, d_tmp.data_ptr(), tmp_bytes, st) == EARG     # beyond the reserved room (32)
    assert L.rbg_tally_add_dev(t.h, d_recs.data_ptr(), R, d_mk.data_ptr(), 33, d_tmp.data_ptr(), tmp_bytes, st) == EARG
    assert t.info() == info0 and _entries(t) == []
    assert L.rbg_tally_add_dev(t.h, d_recs.data_ptr(), 0, d_mk.data_ptr(), 0, d_tmp.data_ptr(), tmp_bytes, st) == 0         # R = 0
    t.reserve(M + 100)
    assert L.rbg_tally_add_dev(t.h, d_recs.data_ptr(), R, d_mk.data_ptr(), M, d_tmp.data_ptr(), tmp_bytes - 8, st) == EARG
    assert L.rbg_tally_add_dev(t.h, None, R, d_mk.data_ptr(), M, d_tmp.data_ptr(), tmp_bytes, st) == EARG
    assert L.rbg_tally_add_dev(t.h, d_recs.data_ptr(), R, d_mk.data_ptr(), M + 100, d_tmp.data_ptr(), tmp_bytes, st) == 0   # an upper bound, not the count
    torch.cuda.synchronize()
    info = t.info()
    assert _entries(t) == TM.sorted_entries(want)
    assert (info["records"], info["elements"], info["dropped"], info["entries"]) == (R, M, 0, len(want)) and info["grows"] == 1
    t.reserve(M)
    assert L.rbg_tally_add_dev(t.h, d_recs.data_ptr(), R, d_mk.data_ptr(), M, d_tmp.data_ptr(), tmp_bytes, st) == 0         # once more: every sum twice
    torch.cuda.synchronize()
    assert _entries(t) == TM.sorted_entries(TM.add_tables(want, want))
    t.close()


# ---- 6. merge --------------------------------------------------------------------------------------------------------------------------

def test_tally_merge(small, toy_reads, want_default):
    rb, o = small
    half = len(toy_reads) // 2
    A, B, E = capi.Tally(rb, 0), capi.Tally(rb, 1000), capi.Tally(rb, 0)
    _feed(rb, A, toy_reads[:half])
    _feed(rb, B, toy_reads[half:])
    a = A.export()
    assert len(a) and _entries(A) == _want(o, toy_reads[:half])
    B.add_entries(a)
    assert _entries(B) == want_default
    E.add_entries(a)
    assert _entries(E) == _entries(A)
    E.add_entries(a[:0])
    assert _entries(E) == _entries(A)
    for t in (A, B, E):
        t.close()


# ---- 7. the tool and the C++ shim ------------------------------------------------------------------------------------------------------

def test_cli_tally(small, toy_reads, data_dir, tmp_path):
    rb, o = small
    idx = os.path.join(data_dir, "small.fa")
    fq = tmp_path / "reads.fq"
    with open(fq, "wb") as f:
        for name, seq in toy_reads:
            f.write(b"@" + name + b" x\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
    out = tmp_path / "out.tsv"
    for args, kw in (([], dict()), (["--heuristic", "--best-strand-only", "--min-seed-length", "30"], dict(heuristic=True, best_strand=True, min_seed_len=30)),
                     (["--batch", "100", "--heuristic", "--device-format"], dict(heuristic=True))):
        rc, stdout, err = _run_rb_markers(args + ["--tally", str(out), idx, str(fq)])
        assert rc == 0 and stdout == "", err
        assert ("ignored" in err) == ("--device-format" in args)
        want = _want(o, toy_reads, **kw)
        assert open(out).read() == TM.entries_tsv(want) and want, args
        os.remove(out)


def test_cpp_shim_tally(small, toy_reads, data_dir, tmp_path):
    rb, o = small
    exe = tmp_path / "tally_shim_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rowbowt_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "tally_shim_check.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "rowbowt_amd"), "-lrbg", "-Wl,-rpath," + os.path.join(ROOT, "rowbowt_amd")])
    recs = [r for r in toy_reads[:120] if r[1]]
    qfile = tmp_path / "q.txt"
    qfile.write_bytes(b"\n".join(s for _, s in recs) + b"\n")
    p = subprocess.run([str(exe), os.path.join(data_dir, "small.fa"), str(qfile)], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    want = _want(o, recs)
    lines = [f"entry {m} {nf} {nr} {ls}" for m, nf, nr, ls in want] + [f"info {len(want)} 1 0", "merged twice 1", "reset 0"]
    assert p.stdout.decode().splitlines() == lines and want
