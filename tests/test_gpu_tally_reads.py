"""The marker tally's per-read mode on the GPU (k_tally_add_reads; rbg_markers_tally_reads, rbg_tally_add_reads_dev, rbg_tally_read_info,
rb_markers --tally-per-read [--tally-drop-conflicts]) against its specification, tests/tally_reads_model.py over the lines rb_markers would print
(tests/rb_markers_model.py::expected_stdout), exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rb_markers_model as RM
import rowbowt_amd as ra
import tally_model as TM
import tally_reads_model as TR
import toy_read_set as TS
from gpu_common import _run_rb_markers
from lmem_model import LmemAsGreedy
from rowbowt_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2**64 - 1
EARG = -4
PR, DS = capi.TALLY_PER_READ, capi.TALLY_DROP_SITE_CONFLICTS
MODES = (0, PR, PR | DS)


@pytest.fixture(scope="module")
def toy_reads(data_dir):
    return TS.renamed(TS.toy_reads(data_dir))     # unique names: the model groups lines by name


def _coins(n):
    b = RM.Booler()
    return np.array([1 if b.get_bool() else 0 for _ in range(n)], dtype=np.uint8)


def _entries(t):
    return [(int(x["marker"]), int(x["n_fwd"]), int(x["n_rev"]), int(x["len_sum"])) for x in t.export()]


def _feed(rb, t, recs, flags, coins=None, **kw):
    """always through rbg_markers_tally_reads itself, flags 0 included"""
    seqs, off = ra.pack_reads([s for _, s in recs])
    if coins is None and kw.get("heuristic"):
        coins = _coins(len(recs))
    coin = None if coins is None else np.ascontiguousarray(coins, dtype=np.uint8)
    p = capi.report_params(**kw)
    rc = rb.L.rbg_markers_tally_reads(rb.h, capi._p(seqs), capi._p(off), len(recs), capi._p(coin), C.byref(p), flags, t.h)
    assert rc == 0, rc


def _run(rb, recs, flags, **kw):
    t = capi.Tally(rb, 0)
    _feed(rb, t, recs, flags, **kw)
    got, info, rinfo = _entries(t), t.info(), t.read_info()
    t.close()
    assert info["dropped"] == 0 and 2 * info["entries"] <= info["capacity"] and info["entries"] == len(got)
    return got, info, rinfo


def _want(text, flags):
    """the model's entries and the counters (info's elements, read_info's last three) for a flag word"""
    if not flags:
        entries = TM.tally_from_stdout(text)[1]
        return entries, sum(nf + nr for _, nf, nr, _ in entries), (0, 0, 0)
    c = TR.read_counts(text, bool(flags & DS))
    return TR.tally_reads_from_stdout(text, bool(flags & DS))[1], c["added"], (c["elements_seen"], c["lost"], c["site_dropped"])


SETS = {"default": dict(), "wsize5": dict(wsize=5), "ftab": dict(wsize=8, ftab_k=6), "lmem": dict(wsize=8, ftab_k=6), "heuristic": dict(heuristic=True),
        "best_strand": dict(heuristic=True, best_strand=True, min_seed_len=30, read_len=101)}
_texts = {}


def _case(o, toy_reads, name):
    """(reads, the library's parameters, the model's stdout -- computed once per parameter set and shared)"""
    kw = SETS[name]
    recs = TS.dozen(toy_reads) if name == "lmem" else [r for r in toy_reads if len(r[1]) >= 6] if name == "ftab" else toy_reads
    if name not in _texts:
        _texts[name] = RM.expected_stdout(LmemAsGreedy(o) if name == "lmem" else o, recs, **kw)
    return recs, dict(kw, lmem=True) if name == "lmem" else kw, _texts[name]


# ---- 1. parity with the model -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SETS))
def test_tally_reads_toy(small, toy_reads, name):
    rb, o = small
    recs, kw, text = _case(o, toy_reads, name)
    results = []
    for flags in MODES:
        got, info, rinfo = _run(rb, recs, flags, **kw)
        want, added, (seen, lost, dropped) = _want(text, flags)
        assert got == want, flags
        assert info["records"] == len(text.splitlines()) and info["elements"] == added
        assert rinfo == dict(reads=len(recs) if flags else 0, elements_seen=seen, lost=lost, site_dropped=dropped), flags
        assert rinfo["elements_seen"] == (added if flags else 0) + rinfo["lost"] + rinfo["site_dropped"]
        results.append(got)
    t = capi.Tally(rb, 0)                                    # flags 0 IS rbg_markers_tally
    seqs, off = ra.pack_reads([s for _, s in recs])
    rb.markers_tally(seqs, off, capi.report_params(**kw), _coins(len(recs)) if kw.get("heuristic") else None, t)
    assert _entries(t) == results[0] and t.read_info() == dict(reads=0, elements_seen=0, lost=0, site_dropped=0)
    t.close()
    if name in ("wsize5", "lmem"):                           # a mode that silently does nothing fails here
        assert results[0] != results[1] and results[1] != results[2] and results[0] != results[2]
    t = capi.Tally(rb, 0)                                    # the binding's flag argument is the same call
    rb.markers_tally(seqs, off, capi.report_params(**kw), _coins(len(recs)) if kw.get("heuristic") else None, t, flags=PR | DS)
    assert _entries(t) == results[2]
    t.close()


# ---- 2. accumulation ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [PR, PR | DS])
def test_tally_reads_accumulates(small, toy_reads, flags, monkeypatch):
    rb, o = small
    recs, kw, text = _case(o, toy_reads, "wsize5")
    want, added, (seen, lost, dropped) = _want(text, flags)
    rwant = dict(reads=len(recs), elements_seen=seen, lost=lost, site_dropped=dropped)
    before = rb.info().hbm_bytes
    t = capi.Tally(rb, 0)
    assert rb.info().hbm_bytes == before + 64 * 32 + 64 and t.read_info() == dict(reads=0, elements_seen=0, lost=0, site_dropped=0)
    half = len(recs) // 2
    _feed(rb, t, recs[:half], flags, **kw)
    _feed(rb, t, recs[half:], flags, **kw)
    assert _entries(t) == want and t.read_info() == rwant and t.info()["elements"] == added
    t.reset()
    assert _entries(t) == [] and t.read_info() == dict(reads=0, elements_seen=0, lost=0, site_dropped=0)
    for chunk in ("150", "1"):                               # many passes; "1" is a pass per read: the rule never looks across passes
        monkeypatch.setenv("RBG_REPORT_CHUNK", chunk)
        _feed(rb, t, recs, flags, **kw)
        assert _entries(t) == want and t.read_info() == rwant, chunk
        t.reset()
    monkeypatch.delenv("RBG_REPORT_CHUNK")
    shuffled = [recs[i] for i in np.random.default_rng(4).permutation(len(recs))]
    for combine in ("0", "1"):
        monkeypatch.setenv("RBG_TALLY_COMBINE", combine)
        _feed(rb, t, recs, flags, **kw)
        assert _entries(t) == want and t.read_info() == rwant, combine
        t.reset()
        _feed(rb, t, shuffled, flags, **kw)
        assert _entries(t) == want and t.read_info() == rwant, combine
        t.reset()
    monkeypatch.delenv("RBG_TALLY_COMBINE")
    _feed(rb, t, [], flags, **kw)                            # N = 0
    assert _entries(t) == [] and t.read_info()["reads"] == 0 and t.info()["records"] == 0
    # one read that has duplicates (and, under the site flag, still adds something), 512 times over
    reads = TR.parse_lines(text)
    for name, lines in reads.items():
        mine = "".join(ln + "\n" for ln in text.splitlines() if ln.split(" ")[0] == name)
        single = _want(mine, flags)
        if single[2][1] > 0 and single[0]:
            break
    else:
        raise AssertionError("no read with duplicates")
    one = recs[int(name)]
    _feed(rb, t, [one] * 512, flags, **kw)
    assert _entries(t) == [(m, 512 * nf, 512 * nr, 512 * ls) for m, nf, nr, ls in single[0]]
    assert t.read_info() == dict(reads=512, elements_seen=512 * single[2][0], lost=512 * single[2][1], site_dropped=512 * single[2][2])
    t.close()
    assert rb.info().hbm_bytes == before


# ---- 3. rbg_tally_add_reads_dev on hand-made records ------------------------------------------------------------------------------------------

def _hand_reads():
    """reads -> records (markers, strand, query_len); every stretch is sorted by rotl4 and unique when it is laid out"""
    rng = np.random.default_rng(41)
    mk = TM.make_marker
    a0, a1 = mk(3, 1000, 0), mk(3, 1000, 1)                                      # two alleles of one site
    top3 = mk(0xFFF, 2**48 - 1, 3)                                               # another allele of marker 2^64 - 1's site
    m, x, z, w = mk(1, 77, 2), mk(1, 78, 0), mk(2, 5, 5), mk(4, 4, 4)
    pool = [mk(int(rng.integers(0, 4)), int(rng.integers(0, 2**40)), 2) for _ in range(40)]   # (one allele: the pool never conflicts)
    big = sorted({mk(5, int(p), 1) for p in rng.integers(0, 2**30, 5200)}, key=TM.rotl4)[:5000]
    p, q = mk(6, 1, 0), mk(6, 2, 0)
    reads = [
        [],                                                                      # no records, as the first read
        [([0, M64, a0, a1], 0, 20)],                                             # one record; keys 0 and 2^64 - 1; both alleles in one record
        [([m], 0, 7), ([m, x], 1, 33), ([m, z], 0, 33)],                         # 7, 33, 33: the second line wins, its strand counts
        [([z, pool[0]], 1, 9), ([], 0, 0), ([], 1, 3)],                          # z again in the NEXT read's first record: it counts twice; empty stretches
        [],                                                                      # no records, in the middle
        [([a0, pool[1]], 0, 15), ([a1], 1, 16), ([pool[1]], 1, 14)],             # the alleles over two records
        [([a1], 0, 12)],                                                         # a1 alone still counts
        [([w], 0, 2**63)], [([w], 1, 2**63 + 5)],                                # two reads: len_sum wraps
        [([w], 0, 2**63), ([w], 1, 2**63 + 5)],                                  # one read: the greater of the two
        [(big, 0, 11), (big[::2], 1, 12)],                                       # 5000 markers, every other one again with a greater query_len
        [([p] if j % 2 else [q], j % 3 == 0, 20 + (j * 7) % 13) for j in range(300)],   # the lmem shape: 300 one-marker records, two markers
        [([M64], 0, 5), ([top3], 1, 6)],                                         # 2^64 - 1 against another allele of its site
    ]
    reads += [[([pool[int(j)] for j in rng.integers(0, 40, 7)], int(i % 2), 30 + i)] for i in range(40)]   # elements across 64-lane / 256-thread borders
    reads += [[], []]                                                            # no records, as the last reads
    return [[(sorted(set(s), key=TM.rotl4), int(st), ql) for s, st, ql in rd] for rd in reads]


def _layout(reads, gap=2):
    """-> (REPORT_SEED records, the marker array with gap words no record points at, rep_off, the same records as rb_markers lines)"""
    flat, recs, rep_off, at, lines = [], [], [0], 0, []
    for i, rd in enumerate(reads):
        for s, strand, qlen in rd:
            flat += [0xDEAD0000 + at] * gap
            at += gap
            recs.append((5, 1, qlen, at, at + len(s), strand, 0))
            flat += s
            at += len(s)
            toks = "".join(f" {(v >> 48) & 0xFFF}/{v & (2**48 - 1)}/{v >> 60}" for v in s) or " ."
            lines.append(f"{i} 5 {'-' if strand else '+'} 1 {qlen}{toks}\n")
        rep_off.append(len(recs))
    flat += [0xDEAD0000 + at] * gap
    return np.array(recs, capi.REPORT_SEED), np.array(flat, dtype=np.uint64), np.array(rep_off, dtype=np.uint64), "".join(lines)


@pytest.fixture(scope="module")
def hand():
    reads = _hand_reads()
    return (len(reads),) + _layout(reads)


@pytest.mark.parametrize("flags", MODES)
def test_tally_add_reads_dev_direct(small, hand, flags):
    import torch
    rb, _ = small
    N, recs, flat, rep_off, text = hand
    R, M = len(recs), int(sum(int(r["mk_end"] - r["mk_begin"]) for r in recs))
    assert M > 7500 and R > 340
    want, added, (seen, lost, dropped) = _want(text, flags)
    if flags:
        assert seen == M and lost > 2500 and (dropped > 0) == bool(flags & DS)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to("cuda:0")
    d_recs, d_mk, d_rep = dev(recs), dev(flat), dev(rep_off)
    L = ra.lib()
    tmp_bytes = L.rbg_tally_add_reads_tmp_bytes(N, R)
    d_tmp = torch.zeros(tmp_bytes, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    t = capi.Tally(rb, 0)
    info0, rinfo0 = t.info(), t.read_info()
    add = lambda recs_p, m_upper, fl, nbytes: L.rbg_tally_add_reads_dev(t.h, recs_p, R, d_rep.data_ptr(), N, d_mk.data_ptr(), m_upper, fl, d_tmp.data_ptr(), nbytes, st)
    assert add(d_recs.data_ptr(), M, flags, tmp_bytes) == EARG                  # beyond the reserved room (32)
    t.reserve(M + 100)
    assert add(d_recs.data_ptr(), M, flags, tmp_bytes - 8) == EARG              # short tmp
    assert add(None, M, flags, tmp_bytes) == EARG                               # no records
    assert add(d_recs.data_ptr(), M, DS, tmp_bytes) == EARG                     # the site flag alone
    assert add(d_recs.data_ptr(), M, flags | 4, tmp_bytes) == EARG              # an unknown flag
    if flags:
        assert L.rbg_tally_add_reads_dev(t.h, d_recs.data_ptr(), R, None, N, d_mk.data_ptr(), M, flags, d_tmp.data_ptr(), tmp_bytes, st) == EARG   # no offsets
    torch.cuda.synchronize()
    assert _entries(t) == [] and t.read_info() == rinfo0 and {k: v for k, v in t.info().items() if k not in ("capacity", "grows")} == \
        {k: v for k, v in info0.items() if k not in ("capacity", "grows")}
    assert L.rbg_tally_add_reads_dev(t.h, d_recs.data_ptr(), 0, d_rep.data_ptr(), 0, d_mk.data_ptr(), 0, flags, d_tmp.data_ptr(), tmp_bytes, st) == 0   # nothing to add
    assert add(d_recs.data_ptr(), M + 100, flags, tmp_bytes) == 0               # M_upper is an upper bound, not the count
    torch.cuda.synchronize()
    info, rinfo = t.info(), t.read_info()
    assert _entries(t) == want
    assert (info["records"], info["elements"], info["dropped"], info["entries"]) == (R, added, 0, len(want))
    assert rinfo == (dict(reads=N, elements_seen=seen, lost=lost, site_dropped=dropped) if flags else rinfo0)
    t.reserve(M)
    assert add(d_recs.data_ptr(), M, flags, tmp_bytes) == 0                     # once more: every sum twice
    torch.cuda.synchronize()
    assert _entries(t) == [(m, 2 * nf, 2 * nr, (2 * ls) & M64) for m, nf, nr, ls in want]
    assert t.read_info() == {k: 2 * v for k, v in rinfo.items()}
    t.close()


def test_tally_add_reads_dev_pinned_cases(small, hand):
    """what the hand-made reads are there for, read off the result entry by entry; N = 1"""
    import torch
    rb, _ = small
    text = hand[4]
    mk = TM.make_marker
    plain, sites = TR.tally_reads_from_stdout(text)[0], TR.tally_reads_from_stdout(text, True)[0]
    a0, a1, top3 = mk(3, 1000, 0), mk(3, 1000, 1), mk(0xFFF, 2**48 - 1, 3)
    assert plain[mk(1, 77, 2)] == (0, 1, 33)                                    # 7, 33, 33: the second line, a '-' line
    assert plain[mk(2, 5, 5)] == (1, 1, 42)                                     # the last record of one read and the first of the next
    assert plain[a0] == (2, 0, 35) and plain[a1] == (2, 1, 48) and a0 not in sites and sites[a1] == (1, 0, 12)
    assert plain[mk(4, 4, 4)] == (1, 2, (2**63 + 2 * (2**63 + 5)) & M64)
    assert plain[M64] == (2, 0, 25) and plain[top3] == (0, 1, 6) and sites[M64] == (1, 0, 20) and top3 not in sites and plain[0] == sites[0] == (1, 0, 20)
    assert plain[mk(6, 1, 0)][0] + plain[mk(6, 1, 0)][1] == 1 and plain[mk(6, 2, 0)][2] == 32
    recs, flat, rep_off, text1 = _layout([[([5, 9], 0, 8), ([9], 1, 8), ([5], 1, 9)]])
    dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to("cuda:0")
    d_recs, d_mk, d_rep = dev(recs), dev(flat), dev(rep_off)
    L = ra.lib()
    tmp_bytes = L.rbg_tally_add_reads_tmp_bytes(1, 3)
    d_tmp = torch.zeros(tmp_bytes, dtype=torch.uint8, device="cuda:0")
    t = capi.Tally(rb, 0)
    assert L.rbg_tally_add_reads_dev(t.h, d_recs.data_ptr(), 3, d_rep.data_ptr(), 1, d_mk.data_ptr(), 4, PR, d_tmp.data_ptr(), tmp_bytes,
                                     torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert _entries(t) == TR.tally_reads_from_stdout(text1)[1] == [(5, 0, 1, 9), (9, 1, 0, 8)]
    assert t.read_info() == dict(reads=1, elements_seen=4, lost=2, site_dropped=0)
    t.close()


# ---- 4. the tool and the C++ shim --------------------------------------------------------------------------------------------------------------

def _write_fq(path, recs):
    with open(path, "wb") as f:
        for name, seq in recs:
            f.write(b"@" + name + b" x\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")


def test_cli_tally_reads(small, toy_reads, data_dir, tmp_path):
    import shutil
    rb, o = small
    idx = os.path.join(data_dir, "small.fa")
    fq, few, out = tmp_path / "reads.fq", tmp_path / "few.fq", tmp_path / "out.tsv"
    _write_fq(fq, toy_reads)
    _write_fq(few, TS.dozen(toy_reads))
    for suf in (".rbwt", ".mab"):
        shutil.copy(idx + suf, tmp_path / ("fx" + suf))
    rb.write_ftab(6, str(tmp_path / "fx.ftab"))
    runs = ((["--batch", "100"], "default", [idx, str(fq)]),
            (["--heuristic", "--best-strand-only", "--min-seed-length", "30"], "best_strand", [idx, str(fq)]),
            (["--lmem", "--ftab", "-w", "8"], "lmem", [str(tmp_path / "fx"), str(few)]))
    for args, name, files in runs:
        text = _case(o, toy_reads, name)[2]
        for mode, flags in (([], 0), (["--tally-per-read"], PR), (["--tally-per-read", "--tally-drop-conflicts"], PR | DS)):
            rc, stdout, err = _run_rb_markers(args + ["--tally", str(out)] + mode + files)
            assert rc == 0 and stdout == "", err
            want = _want(text, flags)[0]
            assert open(out).read() == TM.entries_tsv(want) and want, (args, mode)     # (flags 0: byte-identical to the line model)
            os.remove(out)


def test_cpp_shim_tally_reads(small, toy_reads, data_dir, tmp_path):
    rb, o = small
    exe = tmp_path / "tally_reads_shim_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rowbowt_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "tally_reads_shim_check.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "rowbowt_amd"), "-lrbg", "-Wl,-rpath," + os.path.join(ROOT, "rowbowt_amd")])
    recs = [r for r in toy_reads[:120] if r[1]]
    qfile = tmp_path / "q.txt"
    qfile.write_bytes(b"\n".join(s for _, s in recs) + b"\n")
    names = {n.decode() for n, _ in recs}                    # (no coins in this mode: a read's lines do not depend on the other reads)
    text = "".join(ln + "\n" for ln in _case(o, toy_reads, "wsize5")[2].splitlines() if ln.split(" ")[0] in names)
    for flags in (PR, PR | DS):
        p = subprocess.run([str(exe), os.path.join(data_dir, "small.fa"), str(qfile), "5", str(flags)], capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        want, added, (seen, lost, dropped) = _want(text, flags)
        lines = [f"entry {m} {nf} {nr} {ls}" for m, nf, nr, ls in want] + [f"elements {added}", f"read_info {len(recs)} {seen} {lost} {dropped}", "reset 0 0"]
        assert p.stdout.decode().splitlines() == lines and want and lost
