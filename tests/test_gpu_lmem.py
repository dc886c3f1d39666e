"""GPU parity of the lmem marker seeds (RowBowt::get_markers_lmems, rowbowt.hpp:341-404; needs an MI355X): the C-ABI call
and the device plan/fill pair against tests/lmem_model.py on both rank layouts and both position widths, the rb_markers
--ftab --lmem text byte for byte, and the C++ shim's call sequence."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import golden_values as G
import orc
import rowbowt_amd as ra
from rowbowt_amd import capi
from gpu_common import ROOT, _run_rb_markers, _with_layout
from lmem_model import lmem_records, LmemAsGreedy

pytestmark = pytest.mark.gpu
MAXU = G.MAXU


def _check(rb, o, reads, wsize, max_range, K):
    """rbg_get_markers_lmems == the model, record for record (len(read) records per read, in callback order)"""
    seqs, off = ra.pack_reads(reads)
    seed_off, seeds, mk = rb.get_markers_lmems(seqs, off, wsize, max_range, K)
    assert (seed_off == off).all()
    nmk = 0
    for i, q in enumerate(reads):
        want = lmem_records(o, q, wsize, max_range, K)
        got = seeds[int(seed_off[i]):int(seed_off[i + 1])]
        assert len(got) == len(want) == len(q)
        for g, (wl, wh, wqs, wqe, wm) in zip(got, want):
            assert (int(g[0]), int(g[1]), int(g[2]), int(g[3])) == (wl, wh, wqs, wqe), (i, q, wsize, max_range, K)
            assert mk[int(g[4]):int(g[5])].tolist() == wm, (i, q, wsize, max_range, K)
            nmk += len(wm)
    return len(seeds), nmk


def _toy_reads(data_dir):
    reads = orc.read_fastx(os.path.join(data_dir, "simple_query.fq"))[1] + orc.read_fastx(os.path.join(data_dir, "error_query.fq"))[1]
    return reads + [b"", b"ACG", b"ACGTN", b"N", b"acgtacgtac"]


@pytest.mark.parametrize("layout", [capi.LAYOUT_AUTO, capi.LAYOUT_SLOTS, capi.LAYOUT_RUNS])
def test_lmems_toy_index(data_dir, layout):
    """the reference's toy index with its markers, K = 4 (toy_k4.ftab's k-mer size) and no ftab; wsize around K (quirk 2 sits
    at K - 1, K, K + 1) and a max_range that filters"""
    prefix = os.path.join(data_dir, "small.fa")
    rb = _with_layout(layout, lambda: ra.load_rowbowt(prefix, ra.LoadRbwtFlag.SA | ra.LoadRbwtFlag.MA, device=0))
    o = orc.Oracle.load(prefix, orc.SA | orc.MA)
    reads = _toy_reads(data_dir)
    tot_mk = 0
    for K in (0, 4):
        for wsize in (3, 4, 5, 10, 19):
            for max_range in (MAXU, 3):
                _, nmk = _check(rb, o, reads, wsize, max_range, K)
                tot_mk += nmk
    assert tot_mk > 0
    rb.close()
    o.close()


@pytest.mark.parametrize("layout,pos_bytes", [(capi.LAYOUT_SLOTS, 0), (capi.LAYOUT_RUNS, 0), (capi.LAYOUT_RUNS, 8)])
def test_lmems_synth(synth, layout, pos_bytes):
    """a synthetic pangenome with markers: ragged reads, reads longer than the staging cap (256 symbols: the unstaged walk),
    reads with N, shorter than K, empty"""
    S = synth
    with capi.default_option(capi.OPT_POS_BYTES, pos_bytes):
        rb = _with_layout(layout, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    assert rb.info().pos_bytes == (pos_bytes or 4)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    ms, me, mo, mv = S.markers(wsize=10)
    rb.set_markers(ms, me, mo, mv)
    o.set_markers(ms, me, mo, mv)
    reads = S.sample_reads(150, 120, seed=13, sub_rate=0.4, ragged=True)
    reads += [S.text[100:400].tobytes(), S.text[4100:4400].tobytes() + b"N" + S.text[50:80].tobytes(), b"", b"AC", b"ACGTN", b"NNN",
              S.text[:40].tobytes().lower()]
    nrec, nmk = _check(rb, o, reads, 10, 1000, 0)
    assert nmk > 50
    _check(rb, o, reads, 19, 1000, 12)
    _check(rb, o, reads[:60] + reads[-7:], 5, 4, 6)
    rb.close()
    o.close()


@pytest.mark.parametrize("layout", [capi.LAYOUT_SLOTS, capi.LAYOUT_RUNS])
def test_lmems_device_pair_and_chunks(synth, layout, monkeypatch):
    """rbg_marker_lmems_plan_dev / _fill_dev against the host call (every output slot pre-filled with -1 so that a missed write
    shows), a total given as an upper bound, and the host call over many passes (RBG_LMEM_CHUNK) against one pass"""
    import torch
    S = synth
    rb = _with_layout(layout, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    ms, me, mo, mv = S.markers(wsize=10)
    rb.set_markers(ms, me, mo, mv)
    reads = S.sample_reads(700, 100, seed=31, sub_rate=0.3, ragged=True) + [b"", b"ACGTN", S.text[:300].tobytes()]
    seqs, off = ra.pack_reads(reads)
    N, total = len(reads), int(off[-1])
    for wsize, max_range, K in ((10, 1000, 0), (19, 1000, 12), (7, 5, 8)):
        h_off, h_seeds, h_mk = rb.get_markers_lmems(seqs, off, wsize, max_range, K)
        dev = torch.device("cuda:0")
        d_seqs = torch.from_numpy(np.concatenate([seqs, np.zeros(16 + (-len(seqs)) % 16, np.uint8)])).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        st = torch.cuda.current_stream().cuda_stream
        L = ra.lib()
        for bound in (total, total + 77):
            tmp_bytes = int(L.rbg_marker_lmems_tmp_bytes(N, bound))
            d_tmp = torch.full((tmp_bytes,), -1, dtype=torch.uint8, device=dev)
            d_moff = torch.full((N + 1,), -1, dtype=torch.int64, device=dev)
            assert L.rbg_marker_lmems_plan_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, bound, wsize, max_range, K, d_moff.data_ptr(),
                                               d_tmp.data_ptr(), tmp_bytes, st) == 0
            nmk = int(d_moff[-1].item())
            d_rec = torch.full((6 * total + 6,), -1, dtype=torch.int64, device=dev)
            d_mk = torch.full((nmk + 1,), -1, dtype=torch.int64, device=dev)
            assert L.rbg_marker_lmems_fill_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, bound, wsize, max_range, K, d_tmp.data_ptr(),
                                               d_rec.data_ptr(), d_mk.data_ptr(), st) == 0
            torch.cuda.synchronize()
            rec = d_rec.cpu().numpy().view(np.uint64)
            assert (rec[:6 * total].reshape(total, 6) == h_seeds).all()
            assert rec[6 * total:].view(np.int64).tolist() == [-1] * 6           # nothing past the last record
            got_mk = d_mk.cpu().numpy().view(np.uint64)
            assert (got_mk[:nmk] == h_mk).all() and int(got_mk[nmk].view(np.int64)) == -1
            moff = d_moff.cpu().numpy().view(np.uint64)
            assert (moff == np.array([h_seeds[int(off[i]), 4] if off[i] < total else nmk for i in range(N + 1)], np.uint64)).all()
        assert L.rbg_marker_lmems_plan_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, total, wsize, max_range, K, d_moff.data_ptr(),
                                           d_tmp.data_ptr(), int(L.rbg_marker_lmems_tmp_bytes(N, total)) - 8, st) == -4   # scratch too small
        # the host call in passes of 250 records (sequences never split; the 300-symbol read gets a pass of its own)
        monkeypatch.setenv("RBG_LMEM_CHUNK", "250")
        c_off, c_seeds, c_mk = rb.get_markers_lmems(seqs, off, wsize, max_range, K)
        monkeypatch.delenv("RBG_LMEM_CHUNK")
        assert (c_off == h_off).all() and (c_seeds == h_seeds).all() and (c_mk == h_mk).all()
    rb.close()


def _cli_records(data_dir):
    """test_gpu_cli.test_cli_rb_markers_stdout's 300-read mix"""
    idx = os.path.join(data_dir, "small.fa")
    text = open(idx, "rb").read().split(b"\n", 1)[1].replace(b"\n", b"")
    rng = np.random.default_rng(77)
    recs = []
    for fn in ("simple_query.fq", "error_query.fq"):
        names, seqs = orc.read_fastx(os.path.join(data_dir, fn))
        recs += list(zip(names, seqs))
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    for i in range(300):   # 101 bp reads from either strand, some with errors, lower case and Ns
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


def test_cli_rb_markers_lmem_stdout(data_dir, tmp_path, small):
    import rb_markers_model as RM
    rb, o = small
    idx = os.path.join(data_dir, "small.fa")
    recs = _cli_records(data_dir)
    fq = tmp_path / "reads.fq"
    with open(fq, "wb") as f:
        for name, seq in recs:
            f.write(b"@" + name + b" x\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
    for suf in (".rbwt", ".mab"):
        shutil.copy(idx + suf, tmp_path / ("fx" + suf))
    shutil.copy(os.path.join(ROOT, "tests", "golden", "toy_k4.ftab"), tmp_path / "fx.ftab")
    fx = str(tmp_path / "fx")
    lm = LmemAsGreedy(o)
    rc, out, err = _run_rb_markers(["--ftab", "--lmem", fx, str(fq)])
    assert rc == 0, err
    assert out == RM.expected_stdout(lm, recs, ftab_k=4)
    assert out.count("\n") == 2 * sum(len(s) for _, s in recs)           # m lines per strand, the short read's included (quirk 3)
    for args, kw in ((["-w", "8", "--max-range", "3", "--min-range", "2", "--batch", "7", "--threads", "3"], dict(wsize=8, max_range=3, min_range=2)),
                     (["--heuristic", "--best-strand-only", "-y", "30", "-l", "101"],
                      dict(heuristic=True, best_strand=True, min_seed_len=30, read_len=101)),
                     (["--heuristic", "-y", "25", "--clear-conflicting", "--clear-identical", "-l", "50", "-w", "8"],
                      dict(heuristic=True, min_seed_len=25, clear_conflicting=True, clear_identical=True, read_len=50, wsize=8))):
        rc, out, err = _run_rb_markers(["--ftab", "--lmem"] + args + [fx, str(fq)])
        assert rc == 0, (args, err)
        assert out == RM.expected_stdout(lm, recs, ftab_k=4, **kw), args
    rc, _, err = _run_rb_markers(["--ftab", "--lmem", "-w", "2", fx, str(fq)])
    assert rc == 1 and "wsize cannot be greater" in err                      # rowbowt.hpp:350-353 (k - 1 > wsize)
    rc, _, err = _run_rb_markers(["--lmem", idx, str(fq)])
    assert rc == 1 and "ftab must be enabled!" in err                        # :346-349


def test_cpp_shim_lmems_call_sequence(data_dir, tmp_path, small):
    """rowbowt_gpu.hpp get_markers_lmems replays the reference's calls: per end position the non-empty record, and after a failed
    extension the second call with the empty range, the same q and an empty mbuf"""
    rb, o = small
    exe = tmp_path / "lmem_shim_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rowbowt_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "lmem_shim_check.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "rowbowt_amd"), "-lrbg", "-Wl,-rpath," + os.path.join(ROOT, "rowbowt_amd")])
    idx = os.path.join(data_dir, "small.fa")
    for suf in (".rbwt", ".mab"):
        shutil.copy(idx + suf, tmp_path / ("fx" + suf))
    shutil.copy(os.path.join(ROOT, "tests", "golden", "toy_k4.ftab"), tmp_path / "fx.ftab")
    reads = _toy_reads(data_dir)[:8] + [b"ACGTN", b"ACG"]
    qfile = tmp_path / "q.txt"
    qfile.write_bytes(b"\n".join(reads) + b"\n")
    p = subprocess.run([str(exe), str(tmp_path / "fx"), str(qfile), "10", "1000"], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    want = []
    for q in reads:
        for lo, hi, qs, qe, mk in lmem_records(o, q, 10, 1000, 4):
            want.append(f"{lo} {hi} {qs} {(qe - 1) & MAXU} {' '.join(map(str, mk))}".rstrip())
            if qs > 0:
                want.append(f"1 0 {qs} {(qe - 1) & MAXU}")
        want.append("end")
    assert p.stdout.decode().splitlines() == want
    # without the ftab the reference's error, exit 1
    p = subprocess.run([str(exe), str(tmp_path / "fx"), str(qfile), "10", "1000", "noft"], capture_output=True, timeout=300)
    assert p.returncode == 1 and b"ftab must be enabled!" in p.stderr
