"""rb_build --fasta end to end (needs an MI355X): a FASTA of six records written here -- ACGT-only, mixed case, one with N, one empty, a long header line --
goes through the tool to <out>.rbgpu and <out>.docs; rb_extract --all gives every ACGT-only record back, upper-cased (FASTA -> index -> FASTA); rb_align -s
prints, byte for byte, what it prints on a cache written from the naive arrays of the same text, with reads cut from the records and some across a '#',
which must not be found.  -m with --fasta and a missing file exit 1.  Without --fasta the tool writes what the library writes from the same raw inputs:
the bytes it wrote before the option existed (that path has no changed line; RAW_CACHE_SHA256 is their SHA-256, recorded when the option was added)."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import naive
from rowbowt_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW_CACHE_SHA256 = "0d651caa3ff2a34dc79985d1effe2935b7deb002d96bae377bfd1c36ec31724a"


def _exe(name, args, **kw):
    p = subprocess.run([os.path.join(ROOT, "rowbowt_amd", name)] + [str(a) for a in args], capture_output=True, timeout=300, **kw)
    return p.returncode, p.stdout, p.stderr.decode()


def records():
    rng = np.random.default_rng(6)
    base = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 700).tolist())
    b2 = bytearray(base[:650]); b2[100] = ord("A") if base[100] != ord("A") else ord("C")
    b4 = bytearray(base[50:600]); b4[300:308] = b"NNNNNNNN"
    return [("chr1", "", base), ("chr2", "mixed case", bytes(b2[:300]).lower() + bytes(b2[300:])), ("withN", "", bytes(b4)), ("empty", "nothing here", b""),
            ("long", "a header line " + "x" * 300, base[200:500] + base[:200]), ("last", "", bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 333).tolist()))]


def fasta_bytes(recs, width=61):
    out = b""
    for name, desc, seq in recs:
        out += b">" + name.encode() + ((b" " + desc.encode()) if desc else b"") + b"\n"
        out += b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))
    return out


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("fa")
    recs = records()
    (d / "ref.fa").write_bytes(fasta_bytes(recs))
    rc, out, err = _exe("rb_build", ["--fasta", d / "ref.fa", "-s", "-l", "-o", d / "p"])
    assert rc == 0, err[-800:]
    seqs = [s.upper() for _, _, s in recs]
    text = b"#".join(seqs) + b"\x01"
    starts = np.cumsum([0] + [len(s) + 1 for s in seqs[:-1]]).tolist()
    docs = "".join(f"{n} {s}\n" for (n, _, _), s in zip(recs, starts))
    # the same index from the naive arrays of the same text: what the tool's cache is compared with
    t = np.frombuffer(text, np.uint8)
    sa = naive.suffix_array(t)
    heads, lens, brk = naive.rle(naive.bwt_from_sa(t, sa))
    ssa, esa = naive.run_samples(sa, brk, len(t))
    capi.convert_runs(heads, lens, ssa, esa, out_path=d / "q.rbgpu", docs_text=docs)
    return d, recs, seqs, text, docs


def test_docs_cache_and_round_trip(built):
    d, recs, seqs, text, docs = built
    assert (d / "p.docs").read_text() == docs
    assert (d / "p.rbgpu").read_bytes() == (d / "q.rbgpu").read_bytes()
    rc, out, err = _exe("rb_extract", ["--all", d / "p"])
    assert rc == 0, err[-800:]
    got = {}
    for block in out.split(b">")[1:]:
        head, _, body = block.partition(b"\n")
        got[head.decode()] = body.replace(b"\n", b"")
    for (name, _, _), s in zip(recs, seqs):
        if s and set(s) <= set(b"ACGT"):
            assert got[name] == s, name
    assert sum(1 for s in seqs if s and set(s) <= set(b"ACGT")) == 4


def test_rb_align_is_byte_identical_and_reads_across_a_separator_are_not_found(built):
    d, recs, seqs, text, docs = built
    rng = np.random.default_rng(7)
    reads = []
    for j, s in enumerate(seqs):
        for k in range(5):
            if len(s) >= 40:
                at = int(rng.integers(0, len(s) - 40))
                reads.append((f"r{j}_{k}", s[at:at + 40]))
    cross = []
    at = 0
    for s in seqs[:-1]:
        at += len(s) + 1
        if at >= 21 and at + 20 < len(text):
            cross.append(text[at - 21:at - 1] + text[at:at + 20])      # the bases either side of a '#', the separator left out
    cross = [c for c in cross if set(c) <= set(b"ACGT")]                 # (the two beside the empty record hold its second '#')
    assert len(cross) == 3
    reads += [(f"x{j}", c) for j, c in enumerate(cross)]
    fq = d / "reads.fq"
    fq.write_bytes(b"".join(b"@" + n.encode() + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s in reads))
    rc1, out1, err1 = _exe("rb_align", ["-s", d / "p", fq])
    rc2, out2, err2 = _exe("rb_align", ["-s", d / "q", fq])
    assert rc1 == 0 and rc2 == 0, (err1[-500:], err2[-500:])
    assert out1 == out2 and len(out1) > 0
    lines = out1.decode().split("\n")
    for n, _ in reads:
        head = next(l for l in lines if l.startswith(n + " "))
        assert ("count=0" in head) == n.startswith("x"), head
    assert sum(1 for n, _ in reads if n.startswith("x")) == 3 and sum(1 for n, _ in reads if n.startswith("r")) == 25


def test_what_exits_one(built, tmp_path):
    d = built[0]
    rc, out, err = _exe("rb_build", ["--fasta", d / "ref.fa", "-m", "-o", tmp_path / "m"])
    assert rc == 1 and "a FASTA carries no markers" in err and not (tmp_path / "m.rbgpu").exists()
    rc, out, err = _exe("rb_build", ["--fasta", tmp_path / "missing.fa", "-o", tmp_path / "m"])
    assert rc == 1 and not (tmp_path / "m.rbgpu").exists()
    rc, out, err = _exe("rb_build", ["--fasta", d / "ref.fa"])
    assert rc == 1 and "-o" in err


def test_without_fasta_the_raw_inputs_give_the_same_bytes(tmp_path):
    from synth import SynthIndex
    S = SynthIndex(L=400, H=5, n_sites=12, seed=41)
    pre = tmp_path / "raw"
    (tmp_path / "raw.bwt").write_bytes(naive.expand_bwt(S.heads, S.lens).tobytes())
    pairs = lambda y: np.stack([np.zeros(len(y), np.uint64), np.asarray(y, np.uint64)], axis=1).tobytes()
    (tmp_path / "raw.ssa").write_bytes(pairs(S.ssa))
    (tmp_path / "raw.esa").write_bytes(pairs(S.esa))
    rc, out, err = _exe("rb_build", ["-s", "-o", tmp_path / "out", pre])
    assert rc == 0, err[-500:]
    capi.convert_raw(str(pre) + ".bwt", str(pre) + ".ssa", str(pre) + ".esa", out_path=tmp_path / "lib.rbgpu")
    got = (tmp_path / "out.rbgpu").read_bytes()
    assert got == (tmp_path / "lib.rbgpu").read_bytes()
    assert hashlib.sha256(got).hexdigest() == RAW_CACHE_SHA256
