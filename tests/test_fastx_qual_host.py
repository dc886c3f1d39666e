"""CPU check of the quality spans of rb_align's record scanner (fastx_index.hpp: RecordSpans::qual_begin, the separate qual_arena), in a stand-alone
program under ASan + UBSan (tests/cpp/fastx_qual_dump.cpp): names and sequences against tests/kseq_model.py, the quality strings against what the
input was written from."""
import os
import subprocess

import numpy as np
import pytest

from kseq_model import kseq_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(1 << 20, 1, 1 << 20), (7, 1, 1), (64, 3, 1), (1000, 4, 16), (333, 2, 100)]   # (block bytes, threads, min segment): records split across buffers


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fxq") / "fastx_qual_dump"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                           os.path.join(ROOT, "tests", "cpp", "fastx_qual_dump.cpp"), "-o", str(exe)])

    def run(path, block, threads, minseg):
        p = subprocess.run([str(exe), str(path), str(block), str(threads), str(minseg)], capture_output=True, timeout=120)
        assert p.returncode == 0, (p.stdout[-300:], p.stderr[-600:])
        lines = p.stdout.split(b"\n")
        assert lines[-1] == b"" and lines[-2].startswith(b"rc="), lines[-3:]
        return [tuple(l.split(b"\t")) for l in lines[:-2]], int(lines[-2][3:])
    return run


def _wrap(s, width, eol):
    return eol.join(s[i:i + width] for i in range(0, max(len(s), 1), width)) + eol


def _records(seed, n, fasta_every=0):
    """-> (file bytes, [(name, seq, qual or None)]): quality characters from '#' to 'I' -- none of '@', '+', '>', which kseq would take for a header
    only at the START of a line of the sequence, and never inside a quality string"""
    rng = np.random.default_rng(seed)
    data, recs = b"", []
    for i in range(n):
        m = int(rng.integers(0, 90)) if i % 9 else 0
        seq = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), m))
        qual = bytes(rng.integers(ord("#"), ord("I") + 1, m, dtype=np.uint8).astype(np.uint8))
        name = b"r%d" % i
        eol = b"\r\n" if i % 3 == 1 and m else b"\n"                  # (kseq keeps the lone "\\r" of an empty "\\r\\n" line: empty reads end in "\\n")
        if fasta_every and i % fasta_every == 0:
            data += b">" + name + b" comment" + eol + _wrap(seq, 30 if i % 2 else 1000, eol)
            recs.append((name, seq, None))
            continue
        sw, qw = (1000, 1000) if i % 4 == 0 else (25, 1000) if i % 4 == 1 else (1000, 17) if i % 4 == 2 else (40, 40)
        data += b"@" + name + b" c" + eol + _wrap(seq, sw, eol) + b"+" + (name if i % 5 == 0 else b"") + eol + _wrap(qual, qw, eol)
        recs.append((name, seq, qual))
    return data, recs


@pytest.mark.parametrize("fasta_every", [0, 4], ids=["fastq", "mixed"])
def test_quality_spans(dump, tmp_path, fasta_every):
    """one-line and multi-line quality (alone and beside a multi-line sequence: the two arenas stay apart), "\\r\\n" line ends, empty reads, FASTA records
    mixed with FASTQ, every record split across buffers in some geometry"""
    data, recs = _records(17 + fasta_every, 120, fasta_every)
    want, want_rc = kseq_model(data)
    assert want_rc == -1 and want == [(n, s) for n, s, _ in recs]          # the input means what it was written from
    assert any(q is not None and len(q) > 17 for _, _, q in recs) and b"\r\n" in data
    path = tmp_path / "in.fx"
    path.write_bytes(data)
    for block, threads, minseg in GEOMETRIES:
        got, rc = dump(path, block, threads, minseg)
        assert rc == -1 and len(got) == len(recs), (block, threads, len(got))
        for g, (n, s, q) in zip(got, recs):
            assert g == (n, s, b"-" if q is None else b"=" + q), (block, threads, n)


def test_truncated_quality_keeps_earlier_records(dump, tmp_path):
    data, recs = _records(5, 10)
    path = tmp_path / "t.fq"
    path.write_bytes(data + b"@bad\nACGT\n+\nII\n")
    want, want_rc = kseq_model(path.read_bytes())
    got, rc = dump(path, 64, 2, 1)
    assert rc == want_rc == -2 and [g[:2] for g in got] == want and [g[2] for g in got] == [b"=" + q for _, _, q in recs]
