"""rbg_extract_info, rbg_isa_dev, rbg_extract_dev and rbg_extract (extract.hip, rbg_isa.hpp, capi/extract.ipp) beyond 2^32, at scale and over a collection of
documents -- what the two toy texts of test_gpu_isa.py / test_gpu_extract.py cannot hold (tests/extract_wide_cases.py makes both inputs and every expected
value; tests/test_extract_wide_expected.py runs that half without a device):

  W  a true BWT of n = 4.4e9 symbols, r = 2.46e6, loaded on the run-indexed layout; the load itself chooses 8-byte positions.  tpos and row of the samples
     at and above 2^32, p >> shift with p >= 2^32, a directory of 4.3 M entries of which 83 % repeat their neighbour (empty buckets), a bucket of 809 samples
     (ten probes of the bisection), gaps of up to 78 611 positions (one lane takes 78 610 dependent FL steps), out_off at and above 2^32, host intervals
     across 2^32.  References: the numpy directory over the run-end samples, the CPU oracle over the same run list (LF of a sample's row; the rows hi - j of
     a read's locations SA[hi], SA[hi - 1], ...), and the text itself through TextView.
  D  251 near-copy documents (n = 60 251, 4-byte positions, both layouts): 1 126 samples of the second kind out of non-base BWT runs of up to 206 rows, and
     walks that end at '#', inside a run of N, at "N#", at "##", at the leading N and at the terminator.  References: the naive suffix array's inverse and
     isa_model.expected.

Every comparison is exact.  One device call of a leg takes fewer than extract_wide_cases.STEP_CAP FL steps, counted in numpy before the call.

Wall times on an MI355X (one run; each call with its copies to and from the host): W built on the CPU in 0.9 s (16 threads), loaded in 0.2 s, rbg_extract_prepare
0.08 s.  (b) all 2 456 627 sample positions 0.024 s; before 2 810 samples, 1.6e6 FL steps with one lane of 78 610 dependent steps, 0.057 s.  (c) 358 141
locations, 1.99e9 FL steps, 0.078 s.  (d) 24 911 items, 1.2e8 FL steps, 0.057 s; 1 024 of them on one workgroup 0.077 s.  The same numbers stand in DESIGN 6j,
"Checked, wide"."""
import os
import subprocess
import time

import numpy as np
import pytest
import torch

import extract_wide_cases as C
import rowbowt_amd as ra
from rowbowt_amd import capi
from gpu_common import _with_layout

pytestmark = pytest.mark.gpu
EARG = -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rowbowt_amd", "rb_extract")


class _clock:
    """with _clock("what"): ... -- the wall time of a leg's device calls, printed (pytest -s shows it)"""

    def __init__(self, what):
        self.what = what

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        print(f"\n[extract wide] {self.what}: {time.perf_counter() - self.t0:.3f} s", flush=True)
        return False


@pytest.fixture(scope="module")
def wide():
    """(W, its handle): one load for the module, at the default options but the layout (0.13 s measured at the default k-mer depth: no reason to lower it)"""
    W = C.wide()
    C.wide_shapes(W)
    with _clock("W: rbg_build_from_runs, run-indexed layout"):
        rb = _with_layout(capi.LAYOUT_RUNS, lambda: ra.RowBowt.from_runs(W.heads, W.lens, W.ssa, W.esa, device=0))
    assert int(rb.info().pos_bytes) == 8 and int(rb.info().n) == W.n                         # chosen by the load: no option forces the width
    with _clock("W: rbg_extract_prepare (FL index and ISA sample)"):
        rb.extract_prepare()
    yield W, rb
    rb.close()


def _dev(a, t):
    return torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()


def _extract_dev(rb, pos, length, off, total):
    with torch.cuda.device(int(rb.info().device)):
        d_out = torch.full((total,), C.FILL, dtype=torch.uint8, device="cuda")
        d_got = torch.full((max(len(pos), 1),), -6, dtype=torch.int32, device="cuda")
        rb.extract_dev(_dev(pos.astype(np.uint64), np.int64), _dev(length.astype(np.uint32), np.int32), _dev(off.astype(np.uint64), np.int64), d_out, d_got)
        return d_out.cpu().numpy(), d_got.cpu().numpy().view(np.uint32)[:len(pos)]


def _same(got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    assert len(bad) == 0, (len(bad), bad[:5], np.asarray(got)[bad[:5]], np.asarray(want)[bad[:5]])


# ---- W ------------------------------------------------------------------------------------------------------------------------------------------
def test_info_of_the_wide_index(wide):
    W, rb = wide
    info = rb.extract_info()
    assert info.pop("build_us") >= 0
    assert info == C.wide_info(W) and info["bytes"] == info["samples"] * 2 * 8 + info["dir_entries"] * 8


def test_isa_at_every_sample_and_before_the_samples_with_the_longest_walks(wide):
    W, rb = wide
    x = C.wide_samples()
    with _clock(f"b: rbg_isa_dev at all {len(x.pos)} sample positions, no walk"):
        got = rb.isa(x.pos.astype(np.uint64))
    _same(got, x.row.astype(np.uint64))
    with _clock(f"b: rbg_isa_dev before {len(x.before_pos)} samples, {x.steps} FL steps, the longest lane {x.longest}"):
        got = rb.isa(x.before_pos.astype(np.uint64))
    _same(got, x.before_row.astype(np.uint64))


def test_isa_of_located_positions_is_the_row_they_were_located_from(wide):
    W, rb = wide
    x = C.wide_locate()
    with _clock(f"c: rbg_isa_dev at {len(x.pos)} locations of {x.reads} reads, {x.steps} FL steps, the longest lane {x.longest}"):
        got = rb.isa(x.pos.astype(np.uint64))
    _same(got, x.row.astype(np.uint64))


def test_extract_dev_byte_for_byte_against_the_text(wide, monkeypatch):
    W, rb = wide
    x = C.wide_extract()
    with _clock(f"d: rbg_extract_dev, {len(x.pos)} items, {x.steps} FL steps"):
        out, got = _extract_dev(rb, x.pos, x.length, x.off, len(x.want))
    _same(got, x.got)
    _same(out, x.want)                                                                       # exactly len bytes per item: the fill between them stays
    monkeypatch.setenv("RBG_SAM_GRID_CAP", "1")                                              # one workgroup strides over a reversed stretch
    sub = x.sub
    assert len(x.pos[sub]) <= 1024
    with _clock("d: the first 1024 items reversed, one workgroup"):
        out1, got1 = _extract_dev(rb, x.pos[sub][::-1], x.length[sub][::-1], x.off[sub][::-1], len(x.want))
    monkeypatch.delenv("RBG_SAM_GRID_CAP")
    _same(got1, x.got[sub][::-1])
    end = int(x.off[sub][-1] + x.length[sub][-1])
    _same(out1[:end], x.want[:end])
    assert (out1[end:] == C.FILL).all()


def test_out_off_across_2_32(wide):
    W, rb = wide
    x = C.wide_out_off()
    chunk = 1 << 28
    with torch.cuda.device(int(rb.info().device)):
        d_out = torch.empty((C.BIG_OUT,), dtype=torch.uint8, device="cuda")
        for a in range(0, C.BIG_OUT, chunk):
            d_out[a:a + chunk].fill_(C.FILL)
        d_got = torch.full((len(x.pos),), -6, dtype=torch.int32, device="cuda")
        with _clock("e: rbg_extract_dev, 400 items into 2^32 + 2^20 bytes"):
            rb.extract_dev(_dev(x.pos.astype(np.uint64), np.int64), _dev(x.length.astype(np.uint32), np.int32), _dev(x.off.astype(np.uint64), np.int64), d_out, d_got)
        _same(d_got.cpu().numpy().view(np.uint32), x.got)
        for a, z, want in x.windows:
            _same(d_out[a:z].cpu().numpy(), want)
        # nothing else was written: the bytes that are no longer the fill, counted on the device chunk by chunk (every expected byte is a base or zero)
        written = sum(int((d_out[a:a + chunk] != C.FILL).sum().item()) for a in range(0, C.BIG_OUT, chunk))
        assert written == x.nbytes
        del d_out
        torch.cuda.empty_cache()


def test_host_call_across_2_32_a_whole_haplotype_and_the_end(wide):
    W, rb = wide
    x = C.wide_host()
    p, l, want, g = x["across 2^32"]
    results = []
    assert capi.get_default_option(capi.OPT_EXTRACT_CHUNK) == 128
    with _clock("f: rbg_extract (2^32 - 5000, 10000) at chunks 128, 7 and 1"):
        results.append(rb.extract(p, l))
        for chunk in (7, 1):
            with capi.default_option(capi.OPT_EXTRACT_CHUNK, chunk):
                results.append(rb.extract(p, l))
    for text_out, got in results:
        assert got == g and text_out == want
    p, l, want, g = x["haplotype"]
    with _clock(f"f: rbg_extract of one haplotype unit, {l} bases"):
        text_out, got = rb.extract(p, l)
    assert got == g == l and text_out == want
    p, l, want, g = x["the end"]
    text_out, got = rb.extract(p, l)                                                         # through the terminator and past n
    assert got == g == 299 and text_out == want and text_out[299:] == bytes(701)
    with pytest.raises(ra.RbgError) as ei:
        rb.extract(np.array([3, W.n], np.uint64), np.array([5, 5], np.uint64))
    assert ei.value.code == EARG
    text_out, got = rb.extract(np.array([x["the end"][0], x["across 2^32"][0]], np.uint64), np.array([1000, 100], np.uint64))
    assert got.tolist() == [299, 100] and text_out == x["the end"][2] + x["across 2^32"][2][:100]   # and the next call is right


# ---- D ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[capi.LAYOUT_SLOTS, capi.LAYOUT_RUNS], ids=["slots", "runs"])
def drb(request):
    T = C.docs()
    rb = _with_layout(request.param, lambda: ra.RowBowt.from_runs(T.heads, T.lens, T.ssa, T.esa, device=0))
    assert int(rb.info().pos_bytes) == 4
    rb.extract_prepare()
    yield rb
    rb.close()


def test_documents_info_and_isa_at_every_position(drb):
    T, M = C.docs(), C.docs_model()
    info = drb.extract_info()
    assert info.pop("build_us") >= 0
    assert info == dict(prepared=True, bytes=M.bytes(4), samples=M.samples, shift=M.shift, dir_entries=M.dir_entries, second_kind=M.second_kind, max_gap=M.max_gap)
    assert info["bytes"] == info["samples"] * 2 * 4 + info["dir_entries"] * 4
    _same(drb.isa(np.arange(T.n, dtype=np.uint64)), T.isa.astype(np.uint64))


def test_documents_extract_dev_at_every_position_and_length(drb):
    x = C.docs_extract()
    out, got = _extract_dev(drb, x.pos, x.length, x.off, len(x.want))
    _same(got, x.got)
    _same(out, x.want)


def test_documents_by_their_bounds_from_host_memory(drb):
    pos, length, want = C.docs_documents()
    text_out, got = drb.extract(pos, length)
    assert got.tolist() == [len(w) for w in want]
    at = 0
    for w, l in zip(want, length.tolist()):
        assert text_out[at:at + l] == w + bytes(l - len(w))
        at += l
    assert at == len(text_out)


def test_rb_extract_all_reproduces_the_documents(tmp_path):
    T = C.docs()
    _pos, _length, want = C.docs_documents()
    prefix = str(tmp_path / "docs")
    capi.convert_runs(T.heads, T.lens, T.ssa, T.esa, out_path=prefix + ".rbgpu")
    (tmp_path / "docs.docs").write_text("".join(f"{nm} {s}\n" for nm, s in zip(T.doc_names, T.doc_starts)))
    p = subprocess.run([EXE, "--all", prefix], capture_output=True, timeout=120)
    fasta = lambda nm, seq: b">" + nm.encode() + b"\n" + b"".join(seq[i:i + 60] + b"\n" for i in range(0, len(seq), 60))
    assert p.returncode == 0, p.stderr.decode()[-500:]
    assert p.stdout == b"".join(fasta(nm, w) for nm, w in zip(T.doc_names, want))
    # a warning for every document that holds an N, none for the others (the empty one among them)
    assert p.stderr.decode().count("warning") == sum(len(w) < len(d) for w, d in zip(want, T.docs))
