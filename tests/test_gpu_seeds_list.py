"""GPU parity of the greedy seed lists (RowBowt::get_seeds_greedy rowbowt.hpp:191-215, get_seeds_greedy_w_sample :222-256) and
the toehold checkpoints (find_range_w_toehold_chkpnts :575-606; needs an MI355X): the C-ABI host calls and the device calls
against tests/seeds_model.py on both rank layouts and both position widths, the composition with K3, the consistency with
rbg_greedy_longest_seed, and the C++ shim.  All comparisons are exact integers."""
import os
import subprocess

import numpy as np
import pytest

import golden_values as G
import orc
import rowbowt_amd as ra
from rowbowt_amd import capi
from gpu_common import ROOT, _with_layout
from seeds_model import chkpnt_count, longest_seed, seeds_greedy, toehold_chkpnts
from test_gpu_lmem import _toy_reads

pytestmark = pytest.mark.gpu
MAXU = G.MAXU
QUIRK_READS = [b"", b"N", b"NN", b"ACGTNNACGT", b"ACGNT", b"NACGT", b"ACGTN"]
LAYOUTS_WIDTHS = [(capi.LAYOUT_SLOTS, 0), (capi.LAYOUT_RUNS, 0), (capi.LAYOUT_RUNS, 8)]


def _lists(res):
    """(seed_off, lo, hi, qstart, qend, ssamp) -> per read a list of records"""
    seed_off, cols = res[0], res[1:]
    return [[tuple(int(c[t]) for c in cols) for t in range(int(seed_off[i]), int(seed_off[i + 1]))] for i in range(len(seed_off) - 1)]


def _dev_reads(reads):
    import torch
    seqs, off = ra.pack_reads(reads)
    dev = torch.device("cuda:0")
    d_seqs = torch.from_numpy(np.concatenate([seqs, np.zeros(16 + (-len(seqs)) % 16, np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    return seqs, off, d_seqs, d_off


def _device_pair(rb, reads, min_length, flags, null_ssamp=False):
    """rbg_greedy_seeds_plan_dev + _fill_dev -> (seed_off, lo, hi, qstart, qend, ssamp); every output slot is pre-filled with -1 and
    one more than needed is given, so a missed or a stray write shows"""
    import torch
    _, _, d_seqs, d_off = _dev_reads(reads)
    dev, N, L = d_seqs.device, len(reads), ra.lib()
    st = torch.cuda.current_stream().cuda_stream
    tmp_bytes = int(L.rbg_greedy_seeds_tmp_bytes(N))
    d_tmp = torch.empty(max(tmp_bytes, 1), dtype=torch.uint8, device=dev)
    d_soff = torch.full((N + 1,), -1, dtype=torch.int64, device=dev)
    assert L.rbg_greedy_seeds_plan_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, min_length, flags, d_soff.data_ptr(), d_tmp.data_ptr(),
                                       tmp_bytes, st) == 0
    soff = d_soff.cpu().numpy().view(np.uint64)
    S = int(soff[-1])
    d_out = [torch.full((S + 1,), -1, dtype=torch.int64, device=dev) for _ in range(5)]
    ptrs = [t.data_ptr() for t in d_out]
    if null_ssamp:
        ptrs[4] = None
    assert L.rbg_greedy_seeds_fill_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, min_length, flags, d_soff.data_ptr(), *ptrs, st) == 0
    torch.cuda.synchronize()
    cols = [t.cpu().numpy() for t in d_out]
    assert all(int(c[S]) == -1 for c in cols)                                 # nothing past the last record
    if null_ssamp:
        assert (cols[4] == -1).all()
        cols[4] = np.zeros(S + 1, np.int64)
    return (soff,) + tuple(c[:S].view(np.uint64) for c in cols)


def _check_seed_lists(rb, o, reads, min_lengths, device_pair=True):
    seqs, off = ra.pack_reads(reads)
    nseeds = 0
    for min_length in min_lengths:
        for w_sample in (True, False):
            want = [seeds_greedy(o, q, min_length, w_sample) for q in reads]
            got = _lists(rb.get_seeds_greedy(seqs, off, min_length, w_sample))
            for i, q in enumerate(reads):
                assert got[i] == want[i], (i, q, min_length, w_sample)
            if device_pair:
                dgot = _lists(_device_pair(rb, reads, min_length, capi.SEEDS_W_SAMPLE if w_sample else 0))
                assert dgot == want, (min_length, w_sample)
            nseeds += sum(len(w) for w in want)
    return nseeds


@pytest.mark.parametrize("layout", [capi.LAYOUT_AUTO, capi.LAYOUT_SLOTS, capi.LAYOUT_RUNS])
def test_seed_lists_toy_index(data_dir, layout):
    prefix = os.path.join(data_dir, "small.fa")
    rb = _with_layout(layout, lambda: ra.load_rowbowt(prefix, ra.LoadRbwtFlag.SA | ra.LoadRbwtFlag.MA, device=0))
    o = orc.Oracle.load(prefix, orc.SA | orc.MA)
    reads = _toy_reads(data_dir) + QUIRK_READS
    assert _check_seed_lists(rb, o, reads, (0, 1, 5, 10, 21)) > 200
    # d_ssamp may be NULL without the flag; a flag that does not exist is refused
    assert _lists(_device_pair(rb, reads, 5, 0, null_ssamp=True)) == [seeds_greedy(o, q, 5, False) for q in reads]
    seqs, off = ra.pack_reads(reads)
    so = np.zeros(len(reads) + 1, np.uint64)
    p = capi.VP()
    import ctypes
    assert ra.lib().rbg_get_seeds_greedy(rb.h, seqs.ctypes.data, off.ctypes.data, len(reads), 5, 2, so.ctypes.data, ctypes.byref(p)) == -4
    rb.close()
    o.close()


def _spliced_reads(S, rng, count, joiner):
    """3 to 6 pieces of 12 to 40 symbols cut from the text (ACGT only), joined by one byte: N, or a substituted base"""
    body = S.text[:-1]
    reads = []
    for _ in range(count):
        pieces = []
        for _p in range(int(rng.integers(3, 7))):
            ln = int(rng.integers(12, 41))
            s = int(rng.integers(0, len(body) - ln))
            pieces.append(body[s:s + ln].tobytes())
        q = bytearray(pieces[0])
        for pc in pieces[1:]:
            if joiner == "N":
                q += b"N"
            else:
                q.append(int(rng.choice(list(b"ACGT"))))
            q += pc
        assert set(bytes(q)) <= set(b"ACGTN")
        reads.append(bytes(q))
    return reads


def _synth_reads(S):
    rng = np.random.default_rng(41)
    reads = S.sample_reads(150, 120, seed=13, sub_rate=0.4, ragged=True)
    reads += [S.text[100:400].tobytes(), S.text[4100:4400].tobytes() + b"N" + S.text[50:80].tobytes(), b"", b"AC", b"ACGTN", b"NNN",
              S.text[:40].tobytes().lower(), S.text[700:1000].tobytes()[:150] + b"T" + S.text[1200:1500].tobytes()]
    reads += _spliced_reads(S, rng, 100, "N") + _spliced_reads(S, rng, 50, "sub")
    return reads


@pytest.mark.parametrize("layout,pos_bytes", LAYOUTS_WIDTHS)
def test_seed_lists_synth(synth, layout, pos_bytes):
    """ragged reads with substitutions, reads longer than the 256-symbol staging cap, reads with N, empty reads and spliced
    reads (without those no list is longer than two)"""
    S = synth
    with capi.default_option(capi.OPT_POS_BYTES, pos_bytes):
        rb = _with_layout(layout, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    assert rb.info().pos_bytes == (pos_bytes or 4)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    reads = _synth_reads(S)
    # the condition on the test's own inputs, on the model's output: a quarter of the reads have three or more seeds at min_length 5
    many = sum(len(seeds_greedy(o, q, 5)) >= 3 for q in reads)
    assert 4 * many >= len(reads), (many, len(reads))
    assert _check_seed_lists(rb, o, reads, (0, 5, 10)) > 2000
    _check_seed_lists(rb, o, reads[:40] + reads[-60:], (1, 21), device_pair=False)
    # batches that do not fill a wave
    for cnt in (1, 63, 65):
        _check_seed_lists(rb, o, reads[-cnt:], (5,), device_pair=False)
    rb.close()
    o.close()


@pytest.mark.parametrize("layout", [capi.LAYOUT_SLOTS, capi.LAYOUT_RUNS])
def test_seed_lists_without_toehold_sa(data_dir, synth, layout):
    """flags = 0 works on an index without a toehold SA; with the sample every list is empty (rowbowt.hpp:225), and so is every
    checkpoint list (:579)"""
    S = synth
    prefix = os.path.join(data_dir, "small.fa")
    for rb, o, reads in ((_with_layout(layout, lambda: ra.load_rowbowt(prefix, ra.LoadRbwtFlag.NONE, device=0)), orc.Oracle.load(prefix, orc.NONE),
                          _toy_reads(data_dir) + QUIRK_READS),
                         (_with_layout(layout, lambda: ra.RowBowt.from_runs(S.heads, S.lens, device=0)), orc.Oracle.from_runs(S.heads, S.lens),
                          _synth_reads(S)[-80:])):
        assert not rb.info().has_tsa
        seqs, off = ra.pack_reads(reads)
        for min_length in (0, 5):
            assert _lists(rb.get_seeds_greedy(seqs, off, min_length, False)) == [seeds_greedy(o, q, min_length, False) for q in reads]
            assert _lists(_device_pair(rb, reads, min_length, 0)) == [seeds_greedy(o, q, min_length, False) for q in reads]
            res = rb.get_seeds_greedy(seqs, off, min_length, True)
            assert not res[0].any() and all(len(c) == 0 for c in res[1:])
            dres = _device_pair(rb, reads, min_length, capi.SEEDS_W_SAMPLE)
            assert not dres[0].any()
        res = rb.find_range_w_toehold_chkpnts(seqs, off, 3)
        assert not res[0].any() and all(len(c) == 0 for c in res[1:])
        rb.close()
        o.close()


@pytest.mark.parametrize("layout,pos_bytes", LAYOUTS_WIDTHS)
def test_seed_lists_feed_locate_unchanged(synth, layout, pos_bytes):
    """composition: the filled arrays go unchanged into rbg_locate_plan_dev and rbg_locate_fill_offset_dev (d_sub = d_qstart): for
    every seed the locations are Oracle.locs_at(lo, hi, ssamp) minus qstart; and the first seed of strictly greatest length of
    every list is rbg_greedy_longest_seed's answer"""
    import torch
    S = synth
    with capi.default_option(capi.OPT_POS_BYTES, pos_bytes):
        rb = _with_layout(layout, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    reads = _synth_reads(S)
    seqs, off, d_seqs, d_off = _dev_reads(reads)
    dev, N, L = d_seqs.device, len(reads), ra.lib()
    st = torch.cuda.current_stream().cuda_stream
    min_length, max_hits = 5, 7
    tmp_bytes = int(L.rbg_greedy_seeds_tmp_bytes(N))
    d_tmp = torch.empty(max(tmp_bytes, 1), dtype=torch.uint8, device=dev)
    d_soff = torch.empty(N + 1, dtype=torch.int64, device=dev)
    assert L.rbg_greedy_seeds_plan_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, min_length, capi.SEEDS_W_SAMPLE, d_soff.data_ptr(),
                                       d_tmp.data_ptr(), tmp_bytes, st) == 0
    ns = int(d_soff[-1].item())
    d_lo, d_hi, d_qs, d_qe, d_ss = (torch.empty(ns, dtype=torch.int64, device=dev) for _ in range(5))
    assert L.rbg_greedy_seeds_fill_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, min_length, capi.SEEDS_W_SAMPLE, d_soff.data_ptr(),
                                       d_lo.data_ptr(), d_hi.data_ptr(), d_qs.data_ptr(), d_qe.data_ptr(), d_ss.data_ptr(), st) == 0
    ltmp = int(L.rbg_locate_plan_tmp_bytes(ns))
    d_ltmp = torch.empty(max(ltmp, 1), dtype=torch.uint8, device=dev)
    d_loff = torch.empty(ns + 1, dtype=torch.int64, device=dev)
    assert L.rbg_locate_plan_dev(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), ns, max_hits, d_loff.data_ptr(), d_ltmp.data_ptr(), ltmp, st) == 0
    nl = int(d_loff[-1].item())
    d_locs = torch.full((nl + 1,), -1, dtype=torch.int64, device=dev)
    assert L.rbg_locate_fill_offset_dev(rb.h, d_lo.data_ptr(), d_hi.data_ptr(), d_ss.data_ptr(), ns, max_hits, d_loff.data_ptr(), d_locs.data_ptr(),
                                        d_qs.data_ptr(), None, st) == 0
    torch.cuda.synchronize()
    lo, hi, qs, qe, ss = (t.cpu().numpy().view(np.uint64) for t in (d_lo, d_hi, d_qs, d_qe, d_ss))
    loff, locs = d_loff.cpu().numpy().view(np.uint64), d_locs.cpu().numpy().view(np.uint64)
    assert ns > 600 and nl > ns
    for t in range(ns):
        assert qe[t] > qs[t]                                                   # (min_length 5: no zero-length seed)
        want = [(x - int(qs[t])) & MAXU for x in o.locs_at(int(lo[t]), int(hi[t]), int(ss[t]), max_hits)]
        assert locs[int(loff[t]):int(loff[t + 1])].tolist() == want, t
    # consistency with what exists
    for ml in (0, 5, 10, 40):
        lists = _lists(rb.get_seeds_greedy(seqs, off, ml, True))
        b = rb.greedy_longest_seed(seqs, off, ml)
        for i in range(N):
            best = longest_seed(lists[i])
            got = tuple(int(a[i]) for a in b)
            assert got == (best if best is not None else (1, 0, 0, 0, 0)), (i, ml)
    rb.close()
    o.close()


def _chkpnt_reads(S, o, rng):
    """reads that occur (cut from one haplotype without substitutions) at the lengths the window arithmetic turns on, and reads
    that do not (a substitution that another haplotype happens to carry leaves a read occurring: sorted by the oracle's count)"""
    reads = []
    for m in (0, 1, 2, 3, 4, 10, 11, 19, 20, 21, 38, 39, 40, 41, 58, 60, 61, 64, 65, 128, 129, 257, 300, 301, 400):
        s = int(rng.integers(0, S.L - m))
        reads.append(S.text[s:s + m].tobytes())
    reads += S.sample_reads(60, 150, seed=5, sub_rate=0.0, ragged=True)
    reads += S.sample_reads(30, 120, seed=6, sub_rate=1.0, ragged=True)
    reads += [b"N", b"ACGTN", b"NACGT", S.text[300:700].tobytes() + b"N", b"N" + S.text[300:700].tobytes(), S.text[:40].tobytes().lower()]
    occurring = [q for q in reads if not q or o.count(q) > 0]
    absent = [q for q in reads if q and o.count(q) == 0]
    return occurring, absent


def _device_chkpnts(rb, reads, wsize):
    """the slots call and the walk -> (slot_off, cnt, five arrays)"""
    import torch
    _, _, d_seqs, d_off = _dev_reads(reads)
    dev, N, L = d_seqs.device, len(reads), ra.lib()
    st = torch.cuda.current_stream().cuda_stream
    tmp_bytes = int(L.rbg_toehold_chkpnts_tmp_bytes(N))
    d_tmp = torch.empty(max(tmp_bytes, 1), dtype=torch.uint8, device=dev)
    d_soff = torch.full((N + 1,), -1, dtype=torch.int64, device=dev)
    assert L.rbg_toehold_chkpnts_slots_dev(rb.h, d_off.data_ptr(), N, wsize, d_soff.data_ptr(), d_tmp.data_ptr(), tmp_bytes, st) == 0
    soff = d_soff.cpu().numpy().view(np.uint64)
    S = int(soff[-1])
    d_cnt = torch.full((N,), -1, dtype=torch.int64, device=dev)
    d_out = [torch.full((S + 1,), -1, dtype=torch.int64, device=dev) for _ in range(5)]
    assert L.rbg_find_range_w_toehold_chkpnts_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, wsize, d_soff.data_ptr(), d_cnt.data_ptr(),
                                                  *[t.data_ptr() for t in d_out], st) == 0
    torch.cuda.synchronize()
    cols = [t.cpu().numpy() for t in d_out]
    assert all(int(c[S]) == -1 for c in cols)
    return soff, d_cnt.cpu().numpy().view(np.uint64), [c[:S].view(np.uint64) for c in cols]


@pytest.mark.parametrize("layout,pos_bytes", LAYOUTS_WIDTHS)
def test_toehold_chkpnts(synth, layout, pos_bytes):
    S = synth
    with capi.default_option(capi.OPT_POS_BYTES, pos_bytes):
        rb = _with_layout(layout, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    occurring, absent = _chkpnt_reads(S, o, np.random.default_rng(9))
    assert len(absent) >= 20
    reads = occurring + absent
    assert 2 * len(occurring) >= len(reads)
    seqs, off = ra.pack_reads(reads)
    nrec = 0
    for wsize in (1, 3, 10, 19, 20, 64, 300):
        want = [toehold_chkpnts(o, q, wsize) for q in reads]
        got = _lists(rb.find_range_w_toehold_chkpnts(seqs, off, wsize))
        for i, q in enumerate(reads):
            assert got[i] == want[i], (i, q, wsize)
            assert len(got[i]) == (chkpnt_count(len(q), wsize) if i < len(occurring) else 0), (i, wsize)
        nrec += sum(len(w) for w in want)
        # the device calls: fixed slots from the lengths alone, a count of 0 or all of them
        soff, cnt, cols = _device_chkpnts(rb, reads, wsize)
        for i, q in enumerate(reads):
            assert int(soff[i + 1] - soff[i]) == chkpnt_count(len(q), wsize)
            assert int(cnt[i]) == len(want[i])
            s = int(soff[i])
            assert [tuple(int(c[s + t]) for c in cols) for t in range(int(cnt[i]))] == want[i], (i, wsize)
    assert nrec > 3000
    so = np.zeros(len(reads) + 1, np.uint64)
    import ctypes
    p = capi.VP()
    assert ra.lib().rbg_find_range_w_toehold_chkpnts(rb.h, seqs.ctypes.data, off.ctypes.data, len(reads), 0, so.ctypes.data, ctypes.byref(p)) == -4
    assert ra.lib().rbg_toehold_chkpnts_slots_dev(rb.h, None, 0, 0, so.ctypes.data, None, 0, None) == -4           # wsize == 0
    rb.close()
    o.close()


@pytest.mark.parametrize("layout", [capi.LAYOUT_AUTO, capi.LAYOUT_SLOTS, capi.LAYOUT_RUNS])
def test_toehold_chkpnts_toy_index(data_dir, layout):
    prefix = os.path.join(data_dir, "small.fa")
    rb = _with_layout(layout, lambda: ra.load_rowbowt(prefix, ra.LoadRbwtFlag.SA | ra.LoadRbwtFlag.MA, device=0))
    o = orc.Oracle.load(prefix, orc.SA | orc.MA)
    reads = _toy_reads(data_dir) + QUIRK_READS
    reads += [q[len(q) - m:] for q in reads[:6] for m in (1, 2, 19, 20) if len(q) >= m]
    assert 2 * sum(1 for q in reads if not q or o.count(q)) >= len(reads)
    seqs, off = ra.pack_reads(reads)
    for wsize in (1, 3, 5, 10, 19, 20, 64, 300):
        got = _lists(rb.find_range_w_toehold_chkpnts(seqs, off, wsize))
        for i, q in enumerate(reads):
            assert got[i] == toehold_chkpnts(o, q, wsize), (i, q, wsize)
    rb.close()
    o.close()


def test_cpp_shim_seed_lists(data_dir, tmp_path, small, error_reads):
    """rowbowt_gpu.hpp: GreedyLocateTester (rb_tests.cpp:68-95) as the reference wrote it -- the list first,
    locate_from_longest_seed second -- with the reference's own values, get_seeds_greedy, and find_range_w_toehold_chkpnts on one
    read against the model's values"""
    rb, o = small
    exe = tmp_path / "seeds_shim_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rowbowt_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "seeds_shim_check.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "rowbowt_amd"), "-lrbg", "-Wl,-rpath," + os.path.join(ROOT, "rowbowt_amd")])
    qfile = tmp_path / "q.txt"
    qfile.write_bytes(b"\n".join(error_reads) + b"\n")
    wsize = 7
    chk_read = error_reads[2]
    assert o.count(chk_read) > 0 and chkpnt_count(len(chk_read), wsize) >= 2
    p = subprocess.run([str(exe), os.path.join(data_dir, "small.fa"), str(qfile), "10", chk_read.decode(), str(wsize)], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    want = []
    for q, prefix in zip(error_reads, G.GREEDY_LOCS_PREFIX):
        lfs = seeds_greedy(o, q, 10)
        best = longest_seed(lfs)
        locs = [(x - best[2]) & MAXU for x in o.locs_at(best[0], best[1], best[4])] if best else []
        if prefix is None:
            assert locs == []                                                  # rb_tests.cpp:83-95
        else:
            assert locs[:len(prefix)] == prefix
        want.append("seeds " + " ".join(",".join(map(str, r)) for r in lfs))
        want.append("plain " + " ".join(",".join(map(str, r[:4])) for r in seeds_greedy(o, q, 10, False)))
        want.append("locs " + " ".join(map(str, locs)))
        want.append("batch " + " ".join(",".join(map(str, r)) for r in lfs))
    want.append("chk " + " ".join(",".join(map(str, r)) for r in toehold_chkpnts(o, chk_read, wsize)))
    want.append("empty 0 0")
    assert p.stdout.decode().splitlines() == [w.rstrip() for w in want]


def test_longest_seed_with_the_quad_fetch_switch(synth):
    """RBG_GREEDY_FETCH=quad makes launch_greedy_seed_runs launch the instantiation of k_greedy_seed_runs whose first record of a step is fetched by
    the lane's quad -- one no default process launches.  The switch is read once per process, so the case runs in a child.  rbg_greedy_longest_seed
    at both position widths against the model: the first seed of strictly greatest length of get_seeds_greedy_w_sample's list (rowbowt.hpp:222-256,
    :669-677)."""
    import sys
    if os.environ.get("RBG_GREEDY_FETCH") != "quad":
        r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", f"{__file__}::test_longest_seed_with_the_quad_fetch_switch"],
                           env=dict(os.environ, RBG_GREEDY_FETCH="quad"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
        return
    S = synth
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    reads = [q for q in _synth_reads(S) if len(q) <= 130][:293] + [b"", b"AC", b"ACGTN", b"NNN", S.text[:40].tobytes().lower(), b"A", S.text[300:430].tobytes()]
    assert len(reads) <= 300
    seqs, off = ra.pack_reads(reads)
    want = {ml: [longest_seed(seeds_greedy(o, q, ml)) or (1, 0, 0, 0, 0) for q in reads] for ml in (0, 5, 10, 40)}
    assert sum(w != (1, 0, 0, 0, 0) for w in want[10]) > 100 and any(w == (1, 0, 0, 0, 0) for w in want[40])
    for pos_bytes in (4, 8):
        with capi.default_option(capi.OPT_POS_BYTES, pos_bytes):
            rb = _with_layout(capi.LAYOUT_RUNS, lambda: ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0))
        assert rb.info().rank_layout == capi.LAYOUT_RUNS and rb.info().pos_bytes == pos_bytes
        for ml, w in want.items():
            b = rb.greedy_longest_seed(seqs, off, ml)
            for i in range(len(reads)):
                assert tuple(int(a[i]) for a in b) == w[i], (pos_bytes, ml, i)
        rb.close()
    o.close()
