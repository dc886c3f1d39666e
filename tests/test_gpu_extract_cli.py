"""rb_extract on the reference's fixture index tests/data/greedy_seeding/ref.fa (one document of 20 046 bases), and the C++ shim's extract_prepare / isa /
extract (tests/cpp/extract_shim_check.cpp).  The expected text comes from naive.invert_bwt over the handle's run arrays and the document table, never from the
library's extract."""
import os
import subprocess

import numpy as np
import pytest

import naive
import rowbowt_amd as ra
from rowbowt_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rowbowt_amd", "rb_extract")


@pytest.fixture(scope="module")
def prefix(data_dir):
    return os.path.join(data_dir, "greedy_seeding", "ref.fa")


@pytest.fixture(scope="module")
def doc(prefix):
    """(name, the document's bases) by inverting the BWT the handle holds"""
    rb = ra.load_rowbowt(prefix, ra.LoadRbwtFlag.SA | ra.LoadRbwtFlag.DL, device=0)
    try:
        heads = rb.host_array(capi.ARR_RUN_HEADS).astype(np.uint8)
        start = rb.host_array(capi.ARR_RUN_START)
        nd, starts, names, _size = rb.doc_table()
        n = int(rb.info().n)
    finally:
        rb.close()
    text = naive.invert_bwt(naive.expand_bwt(heads, np.diff(start.astype(np.int64)))).tobytes()
    assert len(text) == n and nd == 1 and int(starts[0]) == 0
    bases = text[:n - 1]
    assert text[n - 1] == 1 and set(bases) <= set(b"ACGT")
    return names[0], bases


def _run(args):
    p = subprocess.run([EXE] + args, capture_output=True, timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


def _fasta(label, seq, width=60):
    return b">" + label.encode() + b"\n" + b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


def test_all_one_name_regions_and_line_width(prefix, doc):
    name, bases = doc
    L = len(bases)
    rc, out, err = _run(["--all", prefix])
    assert rc == 0 and out == _fasta(name, bases) and "warning" not in err, err[-500:]
    rc, out1, err = _run([prefix, name])
    assert rc == 0 and out1 == out and "warning" not in err
    first, last, mid = f"{name}:1-1", f"{name}:{L}-{L}", f"{name}:100-345"
    rc, out, err = _run(["--line-width", "7", prefix, first, last, mid, f"{name}:{L - 9}-{L}"])
    assert rc == 0 and "warning" not in err, err[-500:]
    assert out == (_fasta(first, bases[:1], 7) + _fasta(last, bases[L - 1:], 7) + _fasta(mid, bases[99:345], 7) + _fasta(f"{name}:{L - 9}-{L}", bases[L - 10:], 7))
    # a region over the document's end meets the terminator: written up to it, with a warning
    over = f"{name}:{L - 4}-{L + 1}"
    rc, out, err = _run([prefix, over])
    assert rc == 0 and out == _fasta(over, bases[L - 5:]) and "warning" in err
    rc, out, err = _run([prefix, f"{name}:{L - 4}-{L + 100}"])
    assert rc == 0 and out == _fasta(f"{name}:{L - 4}-{L + 100}", bases[L - 5:]) and "warning" in err


def test_what_exits_one(prefix, doc, tmp_path):
    name, _ = doc
    rc, out, err = _run([prefix, "no_such_document"])
    assert rc == 1 and out == b"" and "no_such_document" in err
    rc, out, err = _run([prefix, f"{name}:5-3"])
    assert rc == 1 and out == b"" and "no region" in err
    rc, out, err = _run([prefix])
    assert rc == 1 and out == b""
    for suf in (".rbwt", ".tsa"):                                                            # an index without its .docs
        os.symlink(prefix + suf, tmp_path / ("idx" + suf))
    rc, out, err = _run([str(tmp_path / "idx"), name])
    assert rc == 1 and out == b"" and "bad file" in err


def test_cpp_shim_extract(prefix, doc, tmp_path):
    name, bases = doc
    exe = tmp_path / "extract_shim_check"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rowbowt_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "extract_shim_check.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "rowbowt_amd"), "-lrbg", "-Wl,-rpath," + os.path.join(ROOT, "rowbowt_amd")])
    (tmp_path / "bases.txt").write_bytes(bases)
    p = subprocess.run([str(exe), prefix, str(tmp_path / "bases.txt")], capture_output=True, timeout=300)
    assert p.returncode == 0 and b"extract shim ok" in p.stdout, p.stdout.decode()[-500:] + p.stderr.decode()[-1500:]
