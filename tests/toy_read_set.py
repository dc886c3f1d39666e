"""Test infrastructure: the read set of the tally tests as a plain function (the same 314 reads as test_gpu_tally.py::toy_reads -- the two toy FASTQ
files, 300 sampled reads of both strands with substitutions, a short and an empty read), and the same reads under unique names."""
import os

import numpy as np

import orc


def toy_reads(data_dir):
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


def renamed(recs):
    """the reads under the names 0, 1, 2, ...: the toy files' names repeat, and the per-read model groups lines by name"""
    return [(str(i).encode(), s) for i, (_, s) in enumerate(recs)]


def dozen(recs):
    """the twelve reads of the lmem checks (test_gpu_tally.py::test_tally_ftab_and_lmem)"""
    return recs[:4] + recs[40:46] + recs[-2:]
