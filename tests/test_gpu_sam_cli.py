"""`rb_align --format sam` (header once, one rbg_align_sam per batch) and the C++ shim's align_sam / sam_header, against tests/sam_model.py: whole stdout,
byte for byte; and `rb_align -s` on the same input, unchanged."""
import gzip
import os
import shutil
import subprocess

import pytest

import orc
import sam_model as SAM
from gpu_common import _run_cli
from test_gpu_text_writers import _text_elems

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PG = b"@PG\tID:rb_align\tPN:rb_align\n"
DOCS = (["ref", "hap1", "hap2"], [0, 10010, 20020])


@pytest.fixture(scope="module")
def idx(data_dir, tmp_path_factory, simple_reads, error_reads):
    d = tmp_path_factory.mktemp("samcli")
    for suf in (".rbwt", ".tsa"):
        shutil.copy(os.path.join(data_dir, "small.fa" + suf), d / ("idx" + suf))
    (d / "idx.docs").write_text("".join(f"{n} {s}\n" for n, s in zip(*DOCS)))
    o = orc.Oracle.load(os.path.join(data_dir, "small.fa"), orc.SA)
    o.set_docs(*DOCS)
    reads = [r for r in (list(simple_reads) + list(error_reads)) if r][:16]
    reads = [SAM.revcomp(q) if i % 2 else q for i, q in enumerate(reads)] + [b"ACGT", b"N" * 25, reads[0][:30]]
    names = [b"q%d" % i for i in range(len(reads))]
    quals = [bytes(35 + (i + 3 * j) % 38 for j in range(len(q))) for i, q in enumerate(reads)]
    yield d, o, names, reads, quals
    o.close()


def _by_batch(o, names, reads, quals, batch, **kw):
    out = b""
    for b0 in range(0, len(reads), batch):
        ql = quals[b0:b0 + batch]
        out += SAM.text(o, names[b0:b0 + batch], reads[b0:b0 + batch], None if any(q is None for q in ql) else ql, **kw)
    return out


def test_rb_align_format_sam(idx):
    d, o, names, reads, quals = idx
    n = o.n
    fq = b"".join(b"@%s desc %d\n%s\n+\n%s\n" % (nm, i, q, ql) for i, (nm, q, ql) in enumerate(zip(names, reads, quals)))
    (d / "q.fq").write_bytes(fq)
    with gzip.open(d / "q.fq.gz", "wb") as f:
        f.write(fq)
    (d / "q.fa").write_bytes(b"".join(b">%s\n%s\n" % (nm, q) for nm, q in zip(names, reads)))
    header = SAM.header(DOCS[0], DOCS[1], n, PG)
    kw = dict(min_length=20, max_hits=16, secondary=False)
    for fname, ql in (("q.fq", quals), ("q.fq.gz", quals), ("q.fa", [None] * len(reads))):
        rc, out, err = _run_cli(["--format", "sam", "--batch", "7", str(d / "idx"), str(d / fname)])
        assert rc == 0, err
        assert out.encode() == header + _by_batch(o, names, reads, ql, 7, **kw), fname
    # the options; and a FASTA record among FASTQ records: QUAL is "*" in the batches that hold it
    mixed = b"".join((b">%s\n%s\n" % (nm, q)) if i == 9 else (b"@%s\n%s\n+\n%s\n" % (nm, q, ql)) for i, (nm, q, ql) in enumerate(zip(names, reads, quals)))
    (d / "mixed.fx").write_bytes(mixed)
    mq = [None if i == 9 else q for i, q in enumerate(quals)]
    rc, out, err = _run_cli(["--format", "sam", "--batch", "7", "--min-seed-length", "12", "--max-hits", "3", "--secondary", str(d / "idx"), str(d / "mixed.fx")])
    assert rc == 0, err
    want = header + _by_batch(o, names, reads, mq, 7, min_length=12, max_hits=3, secondary=True)
    assert out.encode() == want
    assert b"\t*\tNH:" in want and (b"\t256\t" in want or b"\t272\t" in want)      # QUAL "*" on a primary line; secondary lines
    # -s keeps its reference meaning and output
    import numpy as np
    lo, hi, k = (np.array(v, dtype=np.uint64) for v in zip(*[o.find_range_w_toehold(q) for q in reads]))
    rc, out, err = _run_cli(["-s", "--batch", "7", str(d / "idx"), str(d / "q.fq")])
    assert rc == 0, err
    assert out.encode() == b"".join(_text_elems(o, names, lo, hi, k))
    rc, out, err = _run_cli(["--format", "sam", "-s", str(d / "idx"), str(d / "q.fq")])
    assert rc == 1 and out == ""


def test_cpp_shim_align_sam_and_header(idx, data_dir, tmp_path):
    """rowbowt_gpu.hpp align_sam (every overload) and sam_header, instantiated and run (tests/cpp/sam_shim_check.cpp)"""
    d, o, names, reads, quals = idx
    exe = tmp_path / "sam_shim_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rowbowt_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "sam_shim_check.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "rowbowt_amd"), "-lrbg", "-Wl,-rpath," + os.path.join(ROOT, "rowbowt_amd")])
    (tmp_path / "reads.tsv").write_bytes(b"".join(b"%s\t%s\t%s\n" % t for t in zip(names, reads, quals)))
    starts = [20020, 0, 10010]                               # given out of order: d0 goes with the smallest start
    dn = ["d0", "d1", "d2"]
    o.set_docs(dn, starts)
    try:
        header = SAM.header(dn, starts, o.n, b"@PG\tID:sam_shim_check\n")
        for ml, mh, sec, wq in ((20, 16, 0, 1), (20, 16, 0, 0), (12, 3, 1, 1), (12, 3, 1, 0)):
            p = subprocess.run([str(exe), os.path.join(data_dir, "small.fa"), str(tmp_path / "reads.tsv"), ",".join(map(str, starts)), str(ml), str(mh), str(sec), str(wq)],
                               capture_output=True, timeout=300)
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            assert p.stdout == header + SAM.text(o, names, reads, quals if wq else None, ml, mh, bool(sec)), (ml, mh, sec, wq)
    finally:
        o.set_docs(*DOCS)
