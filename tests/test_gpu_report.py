"""GPU parity of rb_markers' report on the device (k_report.hip; rbg_markers_report[_text] and their device steps) against the model of the
reference's worker (tests/rb_markers_model.py), byte for byte."""
import os

import numpy as np
import pytest

import golden_values as G
import orc
import rb_markers_model as RM
import rowbowt_amd as ra
import tally_model as TM
from lmem_model import LmemAsGreedy
from rowbowt_amd import capi
from gpu_common import _run_rb_markers
from synth import SynthIndex

pytestmark = pytest.mark.gpu
M64 = 2**64 - 1


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")


def test_strands(small):
    """k_read_strands: every byte value, lengths around the 16-byte pieces, an input that does not start at offset 0"""
    import torch
    rb, _ = small
    rng = np.random.default_rng(1)
    lens = [0, 1, 2, 15, 16, 17, 31, 33, 100, 101, 0, 256, 7]
    reads = [bytes(range(256))[:n] if n == 256 else bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in lens]
    reads[8] = bytes(rng.choice(np.frombuffer(b"ACGTacgtNnXx-", np.uint8), 100))
    lead = b"\x07" * 21                                    # off[0] = 21: bytes before the first read are not part of the batch
    blob = lead + b"".join(reads)
    off = np.cumsum([len(lead)] + [len(r) for r in reads]).astype(np.uint64)
    N, total = len(reads), int(off[-1] - off[0])
    d_in = _dev(np.frombuffer(blob + b"\0" * (16 + (-len(blob)) % 16), np.uint8))
    d_off = _dev(off)
    L = ra.lib()
    nbytes = L.rbg_read_strands_bytes(total)
    assert nbytes >= 2 * total and nbytes % 16 == 0
    d_out = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_off2 = torch.zeros(2 * N + 1, dtype=torch.int64, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    assert L.rbg_read_strands_dev(rb.h, d_in.data_ptr(), d_off.data_ptr(), N, total, d_out.data_ptr(), d_off2.data_ptr(), st) == 0
    assert L.rbg_read_strands_dev(rb.h, d_in.data_ptr() + 1, d_off.data_ptr(), N, total, d_out.data_ptr(), d_off2.data_ptr(), st) == -4   # alignment
    torch.cuda.synchronize()
    want, woff = b"", [0]
    for r in reads:
        fwd = r.translate(RM.NT)
        want += fwd + fwd.translate(RM.COMP)[::-1]
        woff += [woff[-1] + len(r), woff[-1] + 2 * len(r)]
    assert d_off2.cpu().numpy().tolist() == woff
    got = d_out.cpu().numpy().tobytes()
    assert got[:2 * total] == want
    assert got[(2 * total + 15) // 16 * 16:] == b"\x5A" * (nbytes - (2 * total + 15) // 16 * 16)   # nothing beyond the last 16-byte piece


def _mk(seq, pos, allele):
    return (allele << 60) | (seq << 48) | pos


def _canon_case(rng):
    """synthetic records + markers: every length class next to every other, the contents the filters and the sort can get wrong"""
    lens = [0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 5000]
    order = []
    for rep in range(6):
        order += list(rng.permutation(lens))
    order.insert(17, 70000)
    segs, recs = [], []
    read_len = 101
    for j, n in enumerate(order):
        kind = j % 8
        base_pos = int(rng.integers(0, 2**40))
        if kind == 0:      # heavy duplication
            pool = [_mk(3, base_pos + int(x), int(a)) for x, a in zip(rng.integers(0, 50, 6), rng.integers(0, 16, 6))]
            s = [pool[int(t)] for t in rng.integers(0, len(pool), n)]
        elif kind == 1:    # all equal
            s = [_mk(0xFFF, 2**48 - 1, 15)] * n
        elif kind == 2:    # sorted already, inside one read length, alleles only differing now and then
            s = sorted((_mk(5, base_pos + int(x) % 90, int(a)) for x, a in zip(rng.integers(0, 90, n), rng.integers(0, 3, n))), key=RM.marker_key)
        elif kind == 3:    # reverse sorted, positions further apart than a read
            s = sorted((_mk(5, base_pos + int(x), 1) for x in rng.integers(0, 400, n)), key=RM.marker_key, reverse=True)
        elif kind == 4:    # the sequence changes in the middle
            s = [_mk(1 if t < n // 2 else 2, base_pos + t % 7, t % 16) for t in range(n)]
        elif kind == 5:    # the value 0 first, markers at (0, 0), others that differ only in the allele
            s = ([0, _mk(0, 0, 7)] + [_mk(0, 1 + t // 3, t % 3) for t in range(n)])[:n]
        elif kind == 6:    # pos difference exactly read_len - 1 / read_len
            far = read_len - 1 if (j // 8) % 2 else read_len
            s = ([_mk(9, base_pos, 0), _mk(9, base_pos + far, 0)] + [_mk(9, base_pos + int(x), 2) for x in rng.integers(0, far, n)])[:n]
            rng.shuffle(s)
        else:              # anything
            s = [int(v) for v in rng.integers(0, 2**63, n, dtype=np.uint64) * 2 + rng.integers(0, 2, n, dtype=np.uint64)]
        lo, hi = [(10, 10), (10, 11), (10, 12), (0, M64), (2, 0), (7, 5)][j % 6]    # range_size 1, 2, 3, 0 (wrapped), 2^64 - 1 (wrapped), 2^64 - 1
        segs.append(s)
        recs.append((lo, hi))
    return order, segs, recs, read_len


def _canon_want(s, lo, hi, min_range, read_len, conflicting, identical):
    ms = []
    if ((hi - lo + 1) & M64) >= min_range and s:
        ms = sorted(set(s), key=RM.marker_key)
    if conflicting:
        ms = RM.clear_if_conflicting(ms, read_len)
    if identical:
        ms = RM.filter_identical_pos(ms)
    return ms


@pytest.fixture(scope="module")
def canon_case():
    return _canon_case(np.random.default_rng(11))


@pytest.mark.parametrize("flags", [0, capi.REPORT_CLEAR_CONFLICTING, capi.REPORT_CLEAR_IDENTICAL, capi.REPORT_CLEAR_CONFLICTING | capi.REPORT_CLEAR_IDENTICAL])
def test_canon(small, canon_case, flags, monkeypatch):
    """k_seed_canon / k_seed_canon_big driven directly: sorted(set(..)) and the two filters of the model, for every group width the same"""
    import torch
    rb, _ = small
    order, segs, recs, read_len = canon_case
    min_range = 2
    gap = 3                                               # untouched words between the segments
    flat, seeds, at = [], [], 0
    for s, (lo, hi) in zip(segs, recs):
        flat += [0xDEADBEEF00000000 + at] * gap
        at += gap
        seeds.append((lo, hi, 5, 25, at, at + len(s)))
        flat += s
        at += len(s)
    flat += [0xDEADBEEF00000000 + at] * gap
    h_mk = np.array(flat, dtype=np.uint64)
    h_seeds = np.array(seeds, dtype=np.uint64)
    S = len(seeds)
    L = ra.lib()
    tmp_bytes = L.rbg_marker_seeds_canon_tmp_bytes(S)
    st = torch.cuda.current_stream().cuda_stream
    want = [_canon_want(s, lo, hi, min_range, read_len, bool(flags & capi.REPORT_CLEAR_CONFLICTING), bool(flags & capi.REPORT_CLEAR_IDENTICAL))
            for s, (lo, hi) in zip(segs, recs)]
    assert sum(1 for w in want if w) > 20 and sum(1 for w, s in zip(want, segs) if s and not w) > 5
    results = []
    for group in ("", "4", "16", "64"):
        if group:
            monkeypatch.setenv("RBG_REPORT_GROUP", group)
        else:
            monkeypatch.delenv("RBG_REPORT_GROUP", raising=False)
        d_mk, d_seeds = _dev(h_mk), _dev(h_seeds)
        d_tmp = torch.zeros(tmp_bytes, dtype=torch.uint8, device="cuda:0")
        assert L.rbg_marker_seeds_canon_dev(rb.h, d_seeds.data_ptr(), S, d_mk.data_ptr(), min_range, flags, read_len, d_tmp.data_ptr(), tmp_bytes, st) == 0
        torch.cuda.synchronize()
        g_mk = d_mk.cpu().numpy().view(np.uint64)
        g_seeds = d_seeds.cpu().numpy().view(np.uint64).reshape(S, 6)
        assert (g_seeds[:, :5] == h_seeds[:, :5]).all()
        out = []
        for j in range(S):
            b, e = int(g_seeds[j, 4]), int(g_seeds[j, 5])
            assert b <= e <= int(h_seeds[j, 5])
            got = g_mk[b:e].tolist()
            assert got == want[j], (group, j, order[j], len(got), len(want[j]))
            out.append(got)
            assert (g_mk[b - gap:b] == h_mk[b - gap:b]).all()                       # the words between the segments ...
        assert (g_mk[-gap:] == h_mk[-gap:]).all()
        keep = np.ones(len(h_mk), bool)
        for j in range(S):
            keep[int(h_seeds[j, 4]):int(h_seeds[j, 5])] = False
        assert (g_mk[keep] == h_mk[keep]).all()                                      # ... and everything outside every segment: untouched
        results.append((out, g_seeds[:, 5].tolist()))
    assert all(r == results[0] for r in results[1:])
    assert L.rbg_marker_seeds_canon_dev(rb.h, d_seeds.data_ptr(), S, d_mk.data_ptr(), min_range, flags, read_len, d_tmp.data_ptr(), tmp_bytes - 8, st) == -4


# ---- the report against the model on the toy fixture ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def toy_reads(data_dir):
    """the read set of test_cli_rb_markers_stdout"""
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


def _render(recs, seed_off, seeds, mk):
    """rbg_markers_report's records through the model's line format"""
    out = []
    for i, (name, _) in enumerate(recs):
        for s in seeds[int(seed_off[i]):int(seed_off[i + 1])]:
            ms = mk[int(s["mk_begin"]):int(s["mk_end"])].tolist()
            line = f"{name.decode()} {int(s['range_size'])} {'-' if s['strand'] else '+'} {int(s['query_start'])} {int(s['query_len'])}"
            line += "".join(f" {RM.get_seq(m)}/{G.get_pos(m)}/{G.get_allele(m)}" for m in ms) if ms else " ."
            out.append(line + "\n")
    return "".join(out)


def _both(rb, recs, want, **kw):
    seqs, off = ra.pack_reads([s for _, s in recs])
    names = [n for n, _ in recs]
    params = capi.report_params(**kw)
    coins = _coins(len(recs)) if kw.get("heuristic") else None
    text = rb.markers_report_text(seqs, off, names, params, coins).decode()
    assert text == want, kw
    seed_off, seeds, mk = rb.markers_report(seqs, off, params, coins)
    assert _render(recs, seed_off, seeds, mk) == want, kw
    assert not len(seeds) or int(seeds["mk_end"][-1]) == len(mk)
    return text


PARAM_SETS = [dict(), dict(wsize=10, max_range=3, min_range=2), dict(wsize=5), dict(heuristic=True),
              dict(heuristic=True, best_strand=True, min_seed_len=30, read_len=101),
              dict(heuristic=True, min_seed_len=25, clear_conflicting=True, clear_identical=True, read_len=50, wsize=8)]


@pytest.mark.parametrize("kw", PARAM_SETS, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()) or "default")
def test_report_toy(small, toy_reads, kw):
    rb, o = small
    want = RM.expected_stdout(o, toy_reads, **kw)
    text = _both(rb, toy_reads, want, **kw)
    if not kw:
        assert " + 0 20 0/289/0\n" in text


def test_report_ftab_and_lmem(small, toy_reads):
    rb, o = small
    long_recs = [r for r in toy_reads if len(r[1]) >= 6]
    _both(rb, long_recs, RM.expected_stdout(o, long_recs, wsize=8, ftab_k=6), wsize=8, ftab_k=6)
    _both(rb, long_recs, RM.expected_stdout(o, long_recs, heuristic=True, best_strand=True, min_seed_len=20, ftab_k=6), heuristic=True, best_strand=True,
          min_seed_len=20, ftab_k=6)
    dozen = toy_reads[:4] + toy_reads[40:46] + toy_reads[-2:]
    lm = LmemAsGreedy(o)
    _both(rb, dozen, RM.expected_stdout(lm, dozen, wsize=8, ftab_k=6), wsize=8, ftab_k=6, lmem=True)
    _both(rb, dozen, RM.expected_stdout(lm, dozen, wsize=8, ftab_k=6, heuristic=True, best_strand=True, min_seed_len=30), wsize=8, ftab_k=6, lmem=True,
          heuristic=True, best_strand=True, min_seed_len=30)


def test_report_edges(small, toy_reads, monkeypatch):
    """N = 0 and 1; names of 0, 1, 255 and 300 bytes; a batch forced through several passes; a coin array of mixed bits (the model's own stream), and
    no coin array = every read forward first"""
    rb, o = small
    seqs, off = ra.pack_reads([])
    assert rb.markers_report_text(seqs, off, [], capi.report_params()) == b""
    so, seeds, mk = rb.markers_report(seqs, off, capi.report_params())
    assert so.tolist() == [0] and len(seeds) == 0 and len(mk) == 0
    one = [toy_reads[0]]
    _both(rb, one, RM.expected_stdout(o, one))
    nothing = [(b"e", b"")]
    _both(rb, nothing, RM.expected_stdout(o, nothing))
    rng = np.random.default_rng(3)
    named = []
    for i, (_, s) in enumerate(toy_reads[:260]):
        n = (0, 1, 255, 300)[i % 4] if i < 200 else 300
        named.append((bytes(rng.integers(ord("a"), ord("z") + 1, n, dtype=np.uint8)), s))
    want = RM.expected_stdout(o, named)
    _both(rb, named, want)
    kw = dict(heuristic=True, best_strand=True, min_seed_len=30)
    want_h = RM.expected_stdout(o, toy_reads, **kw)
    coins = _coins(len(toy_reads))
    assert 0 < int(coins.sum()) < len(coins)
    seqs, off = ra.pack_reads([s for _, s in toy_reads])
    names = [n for n, _ in toy_reads]
    fwd_first = rb.markers_report_text(seqs, off, names, capi.report_params(**kw), None)
    assert fwd_first == rb.markers_report_text(seqs, off, names, capi.report_params(**kw), np.ones(len(toy_reads), np.uint8))
    for chunk in ("150", "1000", "1"):   # several passes (a pass holds at least one read)
        monkeypatch.setenv("RBG_REPORT_CHUNK", chunk)
        _both(rb, toy_reads, want_h, **kw)
        _both(rb, named, want)
    monkeypatch.setenv("RBG_REPORT_CHUNK", "300")
    dozen = toy_reads[:4] + toy_reads[40:46] + toy_reads[-2:]
    _both(rb, dozen, RM.expected_stdout(LmemAsGreedy(o), dozen, wsize=8, ftab_k=6), wsize=8, ftab_k=6, lmem=True)


# ---- the shared seed pass at its pass boundaries --------------------------------------------------------------------------------------------

def _boundary_reads(data_dir):
    """Cuts of small.fa of 7, 16, 33, 50 and 8 bytes in this order: with one read per pass the later passes start at read offsets 7, 23, 56 and 106,
    off the 16-byte grid by 7, 7, 8 and 10; the fifth lets a later pass of two reads (3-4) start off the grid too.  The first cut is shorter than the wsize of 8 the test uses, so no window of it reaches a marker lookup
    (no marker in its pass), and shorter than min_seed_len = 12, so the heuristic settings print nothing for it; the 33- and 50-byte cuts lie over
    variant sites (chosen with the model on the CPU; the test asserts both from the model's output).  The last cut goes in reverse-complemented."""
    text = open(os.path.join(data_dir, "small.fa"), "rb").read().split(b"\n", 1)[1].replace(b"\n", b"")
    cuts = [text[p:p + m] for p, m in ((40, 7), (1840, 16), (270, 33), (2205, 50), (905, 8))]
    cuts[3] = cuts[3].translate(RM.COMP)[::-1]
    return [(f"b{i}".encode(), c) for i, c in enumerate(cuts)]


def _strands(recs):
    out = []
    for _, raw in recs:
        fwd = raw.translate(RM.NT)
        out += [fwd, fwd.translate(RM.COMP)[::-1]]
    return out


@pytest.fixture(scope="module")
def uncombined_singles(data_dir):
    """rbg_get_markers_greedy_seeding with N == 1 for every strand of _boundary_reads in a process of its own under RBG_HOST_COMBINE=0 (the switch is
    read once per process): [[records as lists of 6], markers] per strand"""
    import json
    import subprocess
    import sys
    code = ("import json, os, sys\nsys.path[:0] = [%r, %r]\nimport rowbowt_amd as ra\nimport test_gpu_report as T\n"
            "rb = ra.load_rowbowt(os.path.join(%r, 'small.fa'), ra.LoadRbwtFlag.SA | ra.LoadRbwtFlag.MA, device=0)\nout = []\n"
            "for s in T._strands(T._boundary_reads(%r)):\n    _, seeds, mk = rb.get_markers_greedy_seeding(*ra.pack_reads([s]), 8, 1000, 0)\n"
            "    out.append([seeds.tolist(), mk.tolist()])\nrb.close()\nprint('SINGLES', json.dumps(out))\n") % (
                os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))), data_dir, data_dir)
    p = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], capture_output=True, timeout=120,
                       env=dict(os.environ, RBG_HOST_COMBINE="0"))
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return json.loads([line for line in p.stdout.decode().splitlines() if line.startswith("SINGLES ")][0][8:])


@pytest.mark.parametrize("lmem", [False, True], ids=["greedy", "lmem-ftab6"])
@pytest.mark.parametrize("kw", [dict(wsize=8), dict(wsize=8, heuristic=True, min_seed_len=12)], ids=["default", "heuristic-y12"])
def test_report_pass_boundaries(small, data_dir, uncombined_singles, monkeypatch, lmem, kw):
    """One device pass serves rbg_get_markers_greedy_seeding, rbg_get_markers_lmems and the three report calls.  Records, text and tally must not
    depend on how a batch is cut into passes: one pass, one read per pass (passes that start off the 16-byte grid; a first pass without a marker
    and, in the heuristic settings, without a printed record, before passes with both: mbase == 0 then mbase > 0, a tally pass that adds nothing)
    and two reads per pass as far as the lengths allow (no chunk of bytes cuts 7, 16, 33, 50 into 2 + 2: 55 bytes give reads 0-1, 2, 3, 4, and 60
    bytes give 0-2, 3-4, a later pass of two reads that starts off the grid).  All equal the model fed with the host
    call's own seeds of the 2N strands; those equal the oracle's, the host call in passes of one sequence, and its N == 1 form with the one-read
    combiner on and off."""
    rb, o = small
    recs = _boundary_reads(data_dir)
    assert [len(s) for _, s in recs] == [7, 16, 33, 50, 8]
    ftab_k = 6 if lmem else 0
    strands = _strands(recs)
    pk = ra.pack_reads(strands)
    host = rb.get_markers_lmems if lmem else rb.get_markers_greedy_seeding
    h_off, h_seeds, h_mk = host(*pk, 8, 1000, ftab_k)

    def records(i, off=h_off, seeds=h_seeds, mk=h_mk):
        return [tuple(int(v) for v in s[:4]) + (mk[int(s[4]):int(s[5])].tolist(),) for s in seeds[int(off[i]):int(off[i + 1])]]

    table = {s: records(i) for i, s in enumerate(strands)}
    ref = LmemAsGreedy(o) if lmem else o
    for s in strands:   # the host call against the oracle, record for record
        assert table[s] == [tuple(r[:4]) + (list(r[4]),) for r in ref.markers_greedy_seeding(s, 8, 1000, ftab_k)], s
    if lmem:
        assert (h_off == pk[1]).all()
        monkeypatch.setenv("RBG_LMEM_CHUNK", "1")   # a pass per sequence: every later pass rebases its records' marker offsets
        c_off, c_seeds, c_mk = host(*pk, 8, 1000, ftab_k)
        monkeypatch.delenv("RBG_LMEM_CHUNK")
        assert (c_off == h_off).all() and (c_seeds == h_seeds).all() and (c_mk == h_mk).all()
    else:
        for i, s in enumerate(strands):   # N == 1: through the combiner here, around it in the child process
            one = host(*ra.pack_reads([s]), 8, 1000, 0)
            assert one[0].tolist() == [0, len(table[s])] and records(0, *one) == table[s], i
            u_seeds, u_mk = uncombined_singles[i]
            assert [tuple(r[:4]) + (u_mk[r[4]:r[5]],) for r in u_seeds] == table[s], i
    want = RM.expected_stdout(_FakeSeeds(table), recs, ftab_k=ftab_k, **kw)
    lines = lambda name: [x for x in want.splitlines() if x.startswith(name + " ")]
    assert not any(m for rec in table[strands[0]] + table[strands[1]] for m in rec[4])       # the first read's pass has no marker at all ...
    assert bool(lines("b0")) == (not kw.get("heuristic"))                                     # ... and under min_seed_len no printed record
    assert any(not x.endswith(" .") for x in lines("b2")) and any(not x.endswith(" .") for x in lines("b3"))
    want_tally = TM.tally_from_stdout(want)[1]
    assert want_tally
    seqs, off = ra.pack_reads([s for _, s in recs])
    names = [n for n, _ in recs]
    params = capi.report_params(lmem=lmem, ftab_k=ftab_k, **kw)
    coins = _coins(len(recs)) if kw.get("heuristic") else None
    first = None
    for chunk in (None, "1", "55", "60"):
        if chunk:
            monkeypatch.setenv("RBG_REPORT_CHUNK", chunk)
        text = rb.markers_report_text(seqs, off, names, params, coins).decode()
        seed_off, seeds, mk = rb.markers_report(seqs, off, params, coins)
        t = capi.Tally(rb, 0)
        rb.markers_tally(seqs, off, params, coins, t)
        tally = [(int(x["marker"]), int(x["n_fwd"]), int(x["n_rev"]), int(x["len_sum"])) for x in t.export()]
        t.close()
        assert text == want and _render(recs, seed_off, seeds, mk) == want and tally == want_tally, chunk
        got = (seed_off.tolist(), seeds.tobytes(), mk.tolist())
        first = first or got
        assert got == first and (not len(seeds) or int(seeds["mk_end"][-1]) == len(mk)), chunk


def test_report_dense_markers():
    """a small synthetic index with many markers per row and overlapping window hits: real walks whose segments pass the group widths and, with a
    large max_range, the LDS chunk of the long-segment kernel"""
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
    longest = 0
    for kw in (dict(wsize=1, max_range=M64), dict(wsize=3, max_range=40), dict(wsize=1, max_range=M64, heuristic=True, clear_conflicting=True, clear_identical=True,
                                                                              read_len=200)):
        want = RM.expected_stdout(o, reads, **kw)
        _both(rb, reads, want, **kw)
        longest = max(longest, max(len(line.split(" ")) - 5 for line in want.splitlines()))
    _, raw, _ = rb.get_markers_greedy_seeding(*ra.pack_reads([s.translate(RM.NT) for _, s in reads]), 1, M64)
    assert int((raw[:, 5] - raw[:, 4]).max()) > 4096 and longest > 64   # segments beyond the LDS chunk went in, lists beyond a group came out
    rb.close()
    o.close()


def test_report_without_markers():
    S = SynthIndex(L=1500, H=5, n_sites=30, seed=23)
    rb = ra.RowBowt.from_runs(S.heads, S.lens, S.ssa, S.esa, device=0)
    o = orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa)
    reads = [(f"n{i}".encode(), q) for i, q in enumerate(S.sample_reads(40, 30, seed=7, sub_rate=0.1) + [b"ACNNGT", b""])]
    want = RM.expected_stdout(o, reads, wsize=4)
    text = _both(rb, reads, want, wsize=4)
    assert text and all(line.endswith(" .") for line in text.splitlines())
    rb.close()
    o.close()


def test_cli_device_format(small, toy_reads, data_dir, tmp_path):
    """rb_markers --device-format against --host-format: identical stdout over many windows' worth of batches (--batch 7), in the default mode, the
    heuristic mode and --ftab --lmem; the default mode also against the model"""
    import shutil
    rb, o = small
    idx = os.path.join(data_dir, "small.fa")
    fq = tmp_path / "reads.fq"
    with open(fq, "wb") as f:
        for name, seq in toy_reads:
            f.write(b"@" + name + b" x\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
    for suf in (".rbwt", ".mab"):
        shutil.copy(idx + suf, tmp_path / ("fx" + suf))
    rb.write_ftab(4, str(tmp_path / "fx.ftab"))
    few = tmp_path / "few.fq"
    with open(few, "wb") as f:
        for name, seq in toy_reads[:4] + toy_reads[40:50] + toy_reads[-2:]:
            f.write(b"@" + name + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
    for args in ([idx, str(fq)], ["--heuristic", "--best-strand-only", "-y", "30", idx, str(fq)], ["--ftab", "--lmem", str(tmp_path / "fx"), str(few)]):
        rc_h, out_h, err_h = _run_rb_markers(["--host-format", "--batch", "7"] + args)
        rc_d, out_d, err_d = _run_rb_markers(["--device-format", "--batch", "7"] + args)
        assert rc_h == 0 and rc_d == 0, (err_h, err_d)
        assert out_d == out_h and out_d, args
        assert "counting markers took" in err_d
    rc, out, err = _run_rb_markers(["--device-format", idx, str(fq)])
    assert rc == 0 and out == RM.expected_stdout(o, toy_reads)


def test_canon_capped_grid(small):
    """a grid at its cap of 8192 workgroups, far more than are resident at once, so workgroups that start late still have work (at the width of 16
    lanes chosen here the grid holds 131 072 groups, more than the 40 000 records: no group takes a second grid-stride turn), a scratch buffer
    pre-filled with 0xFF, a mean length next to a width threshold, and a last record that the min_range gate empties: the group width is settled
    before any record is rewritten, every segment is processed exactly once"""
    import torch
    rb, _ = small
    rng = np.random.default_rng(29)
    S = 40000
    lens = rng.integers(0, 5, S)
    lens[:600] = 0
    lens[1000] = 100
    lens[-1] = 0
    lens[-1] = 2 * S + 1500 - int(lens.sum())                # the mean is above 2 per record with the last segment and below it without
    begin = np.concatenate(([0], np.cumsum(lens)))
    total = int(begin[-1])
    assert total - int(lens[-1]) < 2 * S < total and lens[-1] > 64
    h_mk = (rng.integers(0, 40, total, dtype=np.uint64) | (rng.integers(0, 3, total).astype(np.uint64) << np.uint64(48))
            | (rng.integers(0, 2, total).astype(np.uint64) << np.uint64(60)))
    h_seeds = np.zeros((S, 6), np.uint64)
    h_seeds[:, 0], h_seeds[:, 1] = 10, 12
    h_seeds[-1, 1] = 10                                      # range_size 1 < min_range 2
    h_seeds[:, 4], h_seeds[:, 5] = begin[:-1], begin[1:]
    L = ra.lib()
    tmp_bytes = L.rbg_marker_seeds_canon_tmp_bytes(S)
    st = torch.cuda.current_stream().cuda_stream
    d_mk, d_seeds = _dev(h_mk), _dev(h_seeds.reshape(-1))
    d_tmp = torch.full((tmp_bytes,), 0xFF, dtype=torch.uint8, device="cuda:0")     # (the scratch header is the call's to set)
    assert L.rbg_marker_seeds_canon_dev(rb.h, d_seeds.data_ptr(), S, d_mk.data_ptr(), 2, 0, 101, d_tmp.data_ptr(), tmp_bytes, st) == 0
    assert L.rbg_marker_seeds_canon_dev(rb.h, d_seeds.data_ptr(), S, None, 2, 0, 101, d_tmp.data_ptr(), tmp_bytes, st) == -4
    torch.cuda.synchronize()
    g_mk = d_mk.cpu().numpy().view(np.uint64)
    g_seeds = d_seeds.cpu().numpy().view(np.uint64).reshape(S, 6)
    assert int(g_seeds[-1, 5]) == int(g_seeds[-1, 4])
    for j in range(S - 1):
        b = int(begin[j])
        want = sorted(set(h_mk[b:int(begin[j + 1])].tolist()), key=RM.marker_key)
        assert g_mk[b:int(g_seeds[j, 5])].tolist() == want, j


class _FakeSeeds:
    """an 'oracle' whose markers_greedy_seeding answers from a table: the model's worker logic over records of the test's choosing"""

    def __init__(self, table):
        self.table = table

    def markers_greedy_seeding(self, seq, wsize, max_range, ftab_k=0):
        return self.table[seq]


@pytest.mark.parametrize("kw", [dict(), dict(heuristic=True), dict(heuristic=True, best_strand=True, min_seed_len=12, read_len=40),
                                dict(heuristic=True, best_strand=True, min_seed_len=0, read_len=30), dict(heuristic=True, min_seed_len=20)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()) or "default")
def test_select_direct(small, kw):
    """k_report_select driven directly with synthetic records: empty ranges, seeds on both sides of min_seed_len, ties for the longest seed,
    stop-rule arithmetic that wraps, reads without records; against the model's worker over the same records"""
    import ctypes as C
    import torch
    rb, _ = small
    rng = np.random.default_rng(31)
    N, m = 700, 30
    reads, table, seeds, seed_off = [], {}, [], [0]
    for i in range(N):
        raw = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), m)) + f"{i:05d}".encode().translate(bytes.maketrans(b"0123456789", b"ACGTACGTAC"))
        raw = raw[:m + 5]
        fwd = raw.translate(RM.NT)
        rev = fwd.translate(RM.COMP)[::-1]
        for seq in (fwd, rev):
            recs = []
            for _ in range(int(rng.integers(0, 5))):
                qs = int(rng.integers(0, len(seq)))
                qe = qs + int(rng.choice([0, 5, 12, 12, 20, 35]))
                lo = int(rng.integers(1, 50))
                hi = lo - 1 if rng.random() < 0.15 else lo + int(rng.integers(0, 4))
                recs.append((lo, hi, qs, qe, []))
                seeds.append((lo & M64, hi & M64, qs, qe, 0, 0))
            table.setdefault(seq, recs)
            if table[seq] is not recs:   # (a palindromic read: both strands must answer alike)
                del seeds[len(seeds) - len(recs):]
                seeds += [(lo & M64, hi & M64, qs, qe, 0, 0) for lo, hi, qs, qe, _ in table[seq]]
            seed_off.append(len(seeds))
        reads.append((f"r{i}".encode(), raw))
    want = RM.expected_stdout(_FakeSeeds(table), reads, **kw)
    h_seeds = np.array(seeds, dtype=np.uint64).reshape(-1)
    lens = np.array([len(r) for _, r in reads], dtype=np.uint64)
    off2 = np.zeros(2 * N + 1, np.uint64)
    off2[1:] = np.cumsum(np.repeat(lens, 2))
    coins = _coins(N)
    params = capi.report_params(**kw)
    L = ra.lib()
    S = len(seeds)
    d_seeds, d_soff, d_off2, d_coin = _dev(h_seeds), _dev(np.array(seed_off, np.uint64)), _dev(off2), _dev(coins)
    d_rep = torch.zeros(N + 1, dtype=torch.int64, device="cuda:0")
    d_out = torch.zeros(6 * S, dtype=torch.int64, device="cuda:0")
    d_read = torch.zeros(S, dtype=torch.int32, device="cuda:0")
    tmp_bytes = L.rbg_report_select_tmp_bytes(N)
    d_tmp = torch.zeros(tmp_bytes, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    assert L.rbg_report_select_dev(rb.h, d_seeds.data_ptr(), d_soff.data_ptr(), d_off2.data_ptr(), N, d_coin.data_ptr(), C.byref(params), d_rep.data_ptr(),
                                   d_out.data_ptr(), d_read.data_ptr(), d_tmp.data_ptr(), tmp_bytes, st) == 0
    assert L.rbg_report_select_dev(rb.h, d_seeds.data_ptr(), d_soff.data_ptr(), d_off2.data_ptr(), N, d_coin.data_ptr(), C.byref(params), d_rep.data_ptr(),
                                   None, d_read.data_ptr(), d_tmp.data_ptr(), tmp_bytes, st) == -4
    torch.cuda.synchronize()
    rep = d_rep.cpu().numpy().view(np.uint64)
    R = int(rep[-1])
    recs = d_out.cpu().numpy().view(np.uint64)[:6 * R].view(capi.REPORT_SEED)
    assert _render(reads, rep, recs, np.zeros(0, np.uint64)) == want
    who = d_read.cpu().numpy()[:R]
    assert who.tolist() == np.repeat(np.arange(N), np.diff(rep).astype(np.int64)).tolist()
    assert 0 < R < S and want
