"""The text rule of rb_build --fasta (rowbowt_amd/csrc/rbg_fasta_text.hpp), CPU only: the header in a program of its own
(tests/cpp/fasta_text_check.cpp, built with AddressSanitizer and UBSan) against a Python model of the rule -- the name is the header up to its first
whitespace; the sequence loses its line ends and is upper-cased; documents joined by '#', a final 0x01, starts = cumsum(len + 1); refused with RBG_EFORMAT:
a sequence byte <= 0x01, a '#', an empty name, no record, a line that begins with '@' or '+' (FASTQ)."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIO, EFORMAT = -1, -2


def model(data):
    """-> (text, docs_text) or the error code"""
    if any(l[:1] in (b"@", b"+") for l in data.split(b"\n")):       # not FASTA to a scanner that reads FASTQ as well
        return EFORMAT
    recs = [r for r in data.replace(b"\r", b"").split(b">")[1:]] if b">" in data else []
    names = [re.split(rb"\s", r.split(b"\n", 1)[0] + b" ", 1)[:1] if not r[:1].isspace() and r[:1] else [] for r in recs]
    seqs = [(r.split(b"\n", 1) + [b""])[1].replace(b"\n", b"").upper() for r in recs]
    if not recs or any(not n for n in names) or any(c <= 1 or c == ord("#") for s in seqs for c in s):
        return EFORMAT
    starts = np.cumsum([0] + [len(s) + 1 for s in seqs[:-1]]).tolist()
    return b"#".join(seqs) + b"\x01", b"".join(n[0] + b" %d\n" % s for n, s in zip(names, starts))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ft") / "fasta_text_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "fasta_text_check.cpp"), "-o", str(exe), "-lz"])

    def run(path):
        p = subprocess.run([str(exe), str(path)], capture_output=True, timeout=60)
        assert p.returncode == 0, (p.stdout[-300:], p.stderr[-2000:])
        kv = dict(l.split(b"=", 1) for l in p.stdout.splitlines())
        rc = int(kv[b"rc"])
        return (bytes.fromhex(kv[b"text"].decode()), bytes.fromhex(kv[b"docs"].decode())) if rc == 0 else rc
    return run


CASES = {
    "lower case": b">a\nacgtnACGT\n>b\nggcc\n",
    "crlf": b">a desc\r\nACGT\r\nAC\r\n>b\r\nGG\r\n",
    "no final newline": b">a\nACGT\n>b\nGGTT",
    "description": b">chr1 Homo sapiens  chromosome 1\tassembly\nACGT\n>chr2\tx\nTT\n",
    "empty record": b">a\nAC\n>e\n>b\nGT\n",
    "two empty records": b">a\nAC\n>e1\n>e2\n>b\nGT\n",
    "empty first and last": b">e0\n>a\nAC\n>e9\n",
    "N runs": b">a\nACNNNNNNNNNNGT\nNNNN\nAC\n>b\nRYKMacgtn\n",
    "N at both ends": b">a\nNACGTN\n>b\nNN\n",
    "one record": b">only\nACGTACGT\nAC\n",
    "wrapped lines": b">a\n" + b"\n".join(b"ACGTTGCAAC"[i % 7:] for i in range(40)) + b"\n>b\nA\n",
    "high bytes": b">a\nAC\x02\xffGT\n",
}
REFUSED = {
    "byte 1": b">a\nAC\x01GT\n",
    "byte 0": b">a\nAC\x00GT\n",
    "separator": b">a\nAC#GT\n",
    "empty name": b">a\nAC\n>\nGT\n",
    "empty name with description": b">a\nAC\n> desc\nGT\n",
    "no record": b"ACGT\nACGT\n",
    "empty file": b"",
    "fastq": b"@r1\nACGT\n+\nIIII\n",
    "fastq record behind a fasta record": b">a\nACGT\n@r1\nACGT\n+\nIIII\n",
    "sequence line that begins with @": b">a\nACGT\n@CGT\n>b\nAC\n",
    "sequence line that begins with +": b">a\nACGT\n+CGT\nACGT\n>b\nAC\n",
    "truncated quality": b">a\nACGT\n+\nII\n",
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_text_and_docs_follow_the_rule(check, tmp_path, name):
    data = CASES[name]
    want = model(data)
    assert want != EFORMAT and want[0].endswith(b"\x01") and want[0].count(b"\x01") == 1
    for gz in (False, True):
        f = tmp_path / ("x.fa.gz" if gz else "x.fa")
        f.write_bytes(gzip.compress(data) if gz else data)
        assert check(f) == want, (name, gz)


def test_the_model_is_the_shape_of_the_extract_cases():
    text, docs = model(b">d0\nAC\n>d1\n>d2\nGGT\n")
    assert text == b"#".join([b"AC", b"", b"GGT"]) + b"\x01" == b"AC##GGT\x01" and docs == b"d0 0\nd1 3\nd2 4\n"
    assert model(CASES["two empty records"])[0] == b"AC###GT\x01"


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_inputs(check, tmp_path, name):
    assert model(REFUSED[name]) == EFORMAT
    for gz in (False, True):
        f = tmp_path / ("x.fa.gz" if gz else "x.fa")
        f.write_bytes(gzip.compress(REFUSED[name]) if gz else REFUSED[name])
        assert check(f) == EFORMAT, (name, gz)


def test_a_missing_file_is_an_io_error(check, tmp_path):
    assert check(tmp_path / "nothing.fa") == EIO
