"""`rb_align --format sam --extend --extend-right` (one rbg_align_sam_extend_both per batch) and the C++ shim's align_sam_extend_both against the library's own
text for the same batches (tests/test_gpu_sam_extend_both.py holds the library to the model); --extend-right alone is refused; without the flag the tool's
output is rbg_align_sam_extend's."""
import os
import shutil
import subprocess

import pytest

import rowbowt_amd as ra
import sam_model as SAM
from rowbowt_amd import capi
from gpu_common import _run_cli

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PG = b"@PG\tID:rb_align\tPN:rb_align\n"
DOCS = (["ref", "hap1", "hap2"], [0, 10010, 20020])


@pytest.fixture(scope="module")
def idx(data_dir, tmp_path_factory, simple_reads, error_reads):
    d = tmp_path_factory.mktemp("sambothcli")
    for suf in (".rbwt", ".tsa"):
        shutil.copy(os.path.join(data_dir, "small.fa" + suf), d / ("idx" + suf))
    (d / "idx.docs").write_text("".join(f"{n} {s}\n" for n, s in zip(*DOCS)))
    rb = capi.load_rowbowt(os.path.join(data_dir, "small.fa"), capi.LoadRbwtFlag.SA)
    rb.set_docs(*DOCS)
    rb.fl_prepare()
    reads = [r for r in (list(simple_reads) + list(error_reads)) if r][:16]
    sub = []
    for i, q in enumerate(reads[:12]):                                 # substitutions near the right end, near the left end, and both: every walk has something to cross
        q = bytearray(q)
        for p in ((len(q) - 5,), (4, len(q) - 3), (5,))[i % 3]:
            q[p] = ord("ACGT"[("ACGT".index(chr(q[p])) + 1) % 4]) if chr(q[p]) in "ACGT" else ord("A")
        sub.append(bytes(q))
    reads = reads + sub
    reads = [SAM.revcomp(q) if i % 2 else q for i, q in enumerate(reads)] + [b"ACGT", b"N" * 25, reads[0][:30]]
    names = [b"q%d" % i for i in range(len(reads))]
    quals = [bytes(35 + (i + 3 * j) % 38 for j in range(len(q))) for i, q in enumerate(reads)]
    yield d, rb, names, reads, quals
    rb.close()


def _by_batch(rb, names, reads, quals, batch, **kw):
    return b"".join(rb.align_sam_extend(reads[b0:b0 + batch], quals[b0:b0 + batch], names[b0:b0 + batch], **kw) for b0 in range(0, len(reads), batch))


def test_rb_align_extend_right(idx):
    d, rb, names, reads, quals = idx
    (d / "q.fq").write_bytes(b"".join(b"@%s desc %d\n%s\n+\n%s\n" % (nm, i, q, ql) for i, (nm, q, ql) in enumerate(zip(names, reads, quals))))
    header = rb.sam_header(PG)
    base = ["--format", "sam", "--batch", "7"]
    tail = [str(d / "idx"), str(d / "q.fq")]
    rc, out, err = _run_cli(base + ["--extend", "--extend-right", "--min-seed-length", "12"] + tail)
    assert rc == 0, err
    both = _by_batch(rb, names, reads, quals, 7, min_length=12, max_hits=16, secondary=False, max_mismatch=4, right=True)
    left = _by_batch(rb, names, reads, quals, 7, min_length=12, max_hits=16, secondary=False, max_mismatch=4)
    assert out.encode() == header + both and both != left              # the right walks moved something
    for K in (0, 8):
        rc, out, err = _run_cli(base + ["--extend", "--extend-right", "--max-mismatches", str(K), "--secondary", "--max-hits", "3", "--min-seed-length", "12"] + tail)
        assert rc == 0, err
        assert out.encode() == header + _by_batch(rb, names, reads, quals, 7, min_length=12, max_hits=3, secondary=True, max_mismatch=K, right=True), K
    rc, out, err = _run_cli(base + ["--extend-right"] + tail)          # refused without --extend
    assert rc == 1 and out == "" and "--extend" in err
    rc, out, err = _run_cli(base + ["--extend", "--min-seed-length", "12"] + tail)          # without the flag: the left call's text, as before
    assert rc == 0, err
    assert out.encode() == header + left


def test_cpp_shim_align_sam_extend_both(idx, data_dir, tmp_path):
    """rowbowt_gpu.hpp fl_prepare and align_sam_extend_both with the default budget and with a given one (tests/cpp/sam_extend_both_shim_check.cpp)"""
    d, rb, names, reads, quals = idx
    exe = tmp_path / "sam_extend_both_shim_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rowbowt_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "sam_extend_both_shim_check.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "rowbowt_amd"), "-lrbg", "-Wl,-rpath," + os.path.join(ROOT, "rowbowt_amd")])
    (tmp_path / "reads.tsv").write_bytes(b"".join(b"%s\t%s\t%s\n" % t for t in zip(names, reads, quals)))
    starts = [20020, 0, 10010]
    rb.set_docs(["d0", "d1", "d2"], starts)
    try:
        for ml, mh, sec, wq, K in ((20, 16, 0, 1, "default"), (12, 3, 1, 0, "1"), (12, 3, 1, 1, "8")):
            p = subprocess.run([str(exe), os.path.join(data_dir, "small.fa"), str(tmp_path / "reads.tsv"), ",".join(map(str, starts)), str(ml), str(mh), str(sec), str(wq), K],
                               capture_output=True, timeout=300)
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            assert p.stdout == rb.align_sam_extend(reads, quals if wq else None, names, ml, mh, bool(sec), 4 if K == "default" else int(K), right=True), (ml, mh, sec, wq, K)
    finally:
        rb.set_docs(*DOCS)
