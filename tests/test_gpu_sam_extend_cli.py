"""`rb_align --format sam --extend` (one rbg_align_sam_extend per batch) and the C++ shim's align_sam_extend, against tests/sam_extend_model.py: whole stdout,
byte for byte; the two argument errors; and `--format sam` without --extend on the same input, unchanged."""
import os
import shutil
import subprocess

import pytest

import orc
import sam_extend_model as XM
import sam_model as SAM
from gpu_common import _run_cli

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PG = b"@PG\tID:rb_align\tPN:rb_align\n"
DOCS = (["ref", "hap1", "hap2"], [0, 10010, 20020])


@pytest.fixture(scope="module")
def idx(data_dir, tmp_path_factory, simple_reads, error_reads):
    d = tmp_path_factory.mktemp("samextcli")
    for suf in (".rbwt", ".tsa"):
        shutil.copy(os.path.join(data_dir, "small.fa" + suf), d / ("idx" + suf))
    (d / "idx.docs").write_text("".join(f"{n} {s}\n" for n, s in zip(*DOCS)))
    o = orc.Oracle.load(os.path.join(data_dir, "small.fa"), orc.SA)
    o.set_docs(*DOCS)
    reads = [r for r in (list(simple_reads) + list(error_reads)) if r][:16]
    sub = []
    for i, q in enumerate(reads[:8]):                                  # 20 bp reads, one and two substitutions near the left end: the walks have something to cross
        q = bytearray(q)
        for p in ((5,), (0, 6))[i % 2]:
            q[p] = ord("ACGT"[("ACGT".index(chr(q[p])) + 1) % 4]) if chr(q[p]) in "ACGT" else ord("A")
        sub.append(bytes(q))
    reads = reads + sub
    reads = [SAM.revcomp(q) if i % 2 else q for i, q in enumerate(reads)] + [b"ACGT", b"N" * 25, reads[0][:30]]
    names = [b"q%d" % i for i in range(len(reads))]
    quals = [bytes(35 + (i + 3 * j) % 38 for j in range(len(q))) for i, q in enumerate(reads)]
    yield d, o, names, reads, quals
    o.close()


def _by_batch(o, names, reads, quals, batch, model, **kw):
    return b"".join(model(o, names[b0:b0 + batch], reads[b0:b0 + batch], quals[b0:b0 + batch], **kw) for b0 in range(0, len(reads), batch))


def test_rb_align_format_sam_extend(idx):
    d, o, names, reads, quals = idx
    (d / "q.fq").write_bytes(b"".join(b"@%s desc %d\n%s\n+\n%s\n" % (nm, i, q, ql) for i, (nm, q, ql) in enumerate(zip(names, reads, quals))))
    header = SAM.header(DOCS[0], DOCS[1], o.n, PG)
    base = ["--format", "sam", "--batch", "7"]
    tail = [str(d / "idx"), str(d / "q.fq")]
    rc, out, err = _run_cli(base + ["--extend", "--min-seed-length", "12"] + tail)
    assert rc == 0, err
    want = header + _by_batch(o, names, reads, quals, 7, XM.text, min_length=12, max_hits=16, secondary=False, K=4)       # the default is 4
    assert out.encode() == want and any(x in want for x in (b"\tNM:i:1\t", b"\tNM:i:2\t"))
    for K in (0, 8):
        rc, out, err = _run_cli(base + ["--extend", "--max-mismatches", str(K), "--secondary", "--max-hits", "3", "--min-seed-length", "12"] + tail)
        assert rc == 0, err
        assert out.encode() == header + _by_batch(o, names, reads, quals, 7, XM.text, min_length=12, max_hits=3, secondary=True, K=K), K
    # the two argument errors
    rc, out, err = _run_cli(base + ["--extend", "--max-mismatches", "9"] + tail)
    assert rc == 1 and out == "" and "max-mismatches" in err
    rc, out, err = _run_cli(base + ["--max-mismatches", "2"] + tail)
    assert rc == 1 and out == "" and "--extend" in err
    # without --extend not one byte changes
    rc, out, err = _run_cli(base + tail)
    assert rc == 0, err
    assert out.encode() == header + _by_batch(o, names, reads, quals, 7, SAM.text, min_length=20, max_hits=16, secondary=False)


def test_cpp_shim_align_sam_extend(idx, data_dir, tmp_path):
    """rowbowt_gpu.hpp align_sam_extend with its default budget and with a given one, instantiated and run (tests/cpp/sam_extend_shim_check.cpp)"""
    d, o, names, reads, quals = idx
    exe = tmp_path / "sam_extend_shim_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rowbowt_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "sam_extend_shim_check.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "rowbowt_amd"), "-lrbg", "-Wl,-rpath," + os.path.join(ROOT, "rowbowt_amd")])
    (tmp_path / "reads.tsv").write_bytes(b"".join(b"%s\t%s\t%s\n" % t for t in zip(names, reads, quals)))
    starts = [20020, 0, 10010]
    dn = ["d0", "d1", "d2"]
    o.set_docs(dn, starts)
    try:
        for ml, mh, sec, wq, K in ((20, 16, 0, 1, "default"), (12, 3, 1, 0, "1"), (12, 3, 1, 1, "8")):
            p = subprocess.run([str(exe), os.path.join(data_dir, "small.fa"), str(tmp_path / "reads.tsv"), ",".join(map(str, starts)), str(ml), str(mh), str(sec), str(wq), K],
                               capture_output=True, timeout=300)
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            assert p.stdout == XM.text(o, names, reads, quals if wq else None, ml, mh, bool(sec), 4 if K == "default" else int(K)), (ml, mh, sec, wq, K)
    finally:
        o.set_docs(*DOCS)
