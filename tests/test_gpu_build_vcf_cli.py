"""rb_build --fasta --vcf -m end to end (needs an MI355X): the reference's own toy FASTA and VCF go through the tool; rb_align -m and rb_markers on the result
print, read for read, the counts and markers they print on the reference-built tests/data/small.fa (the rows differ: '#' joins the documents here, runs of
ten A there, so seeds of ten bases or fewer may count the pads and are compared on the model-built cache only); the cache is byte for byte the one
rbg_convert_runs_markers writes from the model's arrays; rb_extract --all gives the three haplotypes back; --ma-wsize 5 covers as many rows as the model
says; the refusals of the tool exit 1."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import marker_build_model as MB
import sa_scale_cases as SC
from rowbowt_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "data")
FA, VCF = os.path.join(DATA, "small.fa"), os.path.join(DATA, "small.fa.vcf.gz")


def _exe(name, args):
    p = subprocess.run([os.path.join(ROOT, "rowbowt_amd", name)] + [str(a) for a in args], capture_output=True, timeout=300)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def model_cache(path, w):
    V = MB.vcf_text(FA, VCF, None, w)
    sa = capi.suffix_array(torch.from_numpy(V["text"]).cuda()).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    mk = MB.marker_runs(sa, V["pos"], V["first"], V["val"])
    docs = "".join(f"{n} {s}\n" for n, s in zip(V["names"], V["starts"]))
    capi.convert_runs(*SC.runs_from_sa(V["text"], sa), out_path=path, markers=mk, docs_text=docs)
    return V, sa, mk, docs


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("vcf")
    rc, out, err = _exe("rb_build", ["--fasta", FA, "--vcf", VCF, "-m", "-s", "-l", "-o", d / "x"])
    assert rc == 0, err[-800:]
    assert "skipped sites: 0 indel or MNV, 0 symbolic or non-ACGT, 0 on a contig the FASTA lacks, 0 duplicate position" in err
    return (d,) + model_cache(d / "y.rbgpu", 10)


def test_cache_docs_and_round_trip(built):
    d, V, sa, mk, docs = built
    assert (d / "x.docs").read_text() == docs == "ref 0\nsample0.1.ref 10001\nsample0.2.ref 20002\n"
    assert (d / "x.rbgpu").read_bytes() == (d / "y.rbgpu").read_bytes()
    rc, out, err = _exe("rb_extract", ["--all", d / "x"])
    assert rc == 0, err[-800:]
    got = {b.split("\n", 1)[0].split()[0]: b.split("\n", 1)[1].replace("\n", "") for b in out.split(">")[1:]}
    haps = bytes(V["text"][:-1]).decode().split("#")
    assert got == dict(zip(V["names"], haps)) and len(set(haps)) == 3


def align_records(out):
    """[(name, count, markers line)] of rb_align -m"""
    recs = re.findall(r"^(\S+) \(\d+,\d+\), count=(\d+)\n\tmarkers: (.*)\n", out, flags=re.M)
    assert recs
    return recs


@pytest.mark.parametrize("query", ["simple_query.fq", "error_query.fq"])
def test_rb_align_and_rb_markers_agree_with_the_reference_built_index(built, query):
    d = built[0]
    fq = os.path.join(DATA, query)
    a, b = _exe("rb_align", ["-m", d / "x", fq]), _exe("rb_align", ["-m", FA, fq])
    assert a[0] == b[0] == 0, (a[2][-400:], b[2][-400:])
    assert align_records(a[1]) == align_records(b[1])
    if query == "simple_query.fq":      # (no read of error_query.fq matches as a whole: its lines carry no markers on either index)
        assert any("/" in m for _n, _c, m in align_records(a[1]))
    a, b, c = _exe("rb_markers", [d / "x", fq]), _exe("rb_markers", [FA, fq]), _exe("rb_markers", [d / "y", fq])
    assert a[0] == b[0] == c[0] == 0, (a[2][-400:], b[2][-400:])
    assert a[1] == c[1] and a[1]
    long_seeds = lambda out: [l for l in out.splitlines() if int(l.split()[4]) > 10]      # (a seed of ten bases or fewer may lie in the reference's pads of A)
    assert long_seeds(a[1]) == long_seeds(b[1]) and long_seeds(a[1])
    if query == "simple_query.fq":
        assert any(l.split()[5] != "." for l in long_seeds(a[1]))


def test_a_window_of_five(built, tmp_path):
    rc, out, err = _exe("rb_build", ["--fasta", FA, "--vcf", VCF, "--ma-wsize", "5", "-m", "-s", "-o", tmp_path / "w5"])
    assert rc == 0 and "windows of 5" in err, err[-800:]
    V, sa, mk, docs = model_cache(tmp_path / "m5.rbgpu", 5)
    capi.convert_runs(*SC.runs_from_sa(V["text"], sa), out_path=tmp_path / "m5.rbgpu", markers=mk)
    assert (tmp_path / "w5.rbgpu").read_bytes() == (tmp_path / "m5.rbgpu").read_bytes()
    covered = int((mk[1] - mk[0]).astype(np.int64).sum()) + len(mk[0])
    assert covered == len(MB.covered_rows(sa, V["pos"], V["first"])) == 150 < 300


def test_tool_refusals(tmp_path):
    none = tmp_path / "indels.vcf"      # every site skipped: -m would get no marker array
    none.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts\nref\t5\t.\tGA\tG\t.\t.\t.\tGT\t0|1\n")
    for args, word in ((["--fasta", FA, "--samples", "sample0", "-o", tmp_path / "h"], "--samples and --ma-wsize belong to --vcf"),
                       (["--fasta", FA, "--ma-wsize", "10", "-o", tmp_path / "i"], "--samples and --ma-wsize belong to --vcf"),
                       (["--fasta", FA, "--vcf", none, "-m", "-o", tmp_path / "j"], "there would be no marker array"),
                       (["--vcf", VCF, "-m", "-o", tmp_path / "a", "prefix"], "--vcf needs --fasta and -m"),
                       (["--fasta", FA, "--vcf", VCF, "-o", tmp_path / "b"], "--vcf needs --fasta and -m"),
                       (["--fasta", FA, "-m", "-o", tmp_path / "c"], "a FASTA carries no markers"),
                       (["--fasta", FA, "--vcf", VCF, "-m", "--ma-wsize", "65", "-o", tmp_path / "d"], "--ma-wsize must be 1..64"),
                       (["--fasta", FA, "--vcf", VCF, "-m", "--ma-wsize", "0", "-o", tmp_path / "e"], "--ma-wsize must be 1..64"),
                       (["--fasta", FA, "--vcf", VCF, "-m", "--samples", "nobody", "-o", tmp_path / "f"], "sample nobody is absent"),
                       (["--fasta", FA, "--vcf", tmp_path / "none.vcf", "-m", "-o", tmp_path / "g"], "cannot be opened")):
        rc, out, err = _exe("rb_build", args)
        assert rc == 1 and word in err, (args, err[-400:])
    assert not list(tmp_path.glob("*.rbgpu"))
