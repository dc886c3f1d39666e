"""The haplotype text and the site records of rb_build --fasta --vcf (rowbowt_amd/csrc/rbg_vcf.hpp), CPU only: the header in a program of its
own (tests/cpp/vcf_text_check.cpp, built with AddressSanitizer and UBSan) against the Python model tests/marker_build_model.py::vcf_text -- documents,
.docs text, records, skip counts, and for every refusal the line it names."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import marker_build_model as MB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "data")
EFORMAT = -2
HDR = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t"
FA = ">chr1 first\nACGTACGTACGTACGTACGTACGTACGTAC\n>chr2\nGGGTTTCCCAAAGGGTTTCC\n"      # 30 and 20 bases


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("vt") / "vcf_text_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "vcf_text_check.cpp"), "-o", str(exe), "-lz"])

    def run(fa, vcf, w=10, samples=None):
        p = subprocess.run([str(exe), str(fa), str(vcf), str(w)] + ([",".join(samples)] if samples is not None else []), capture_output=True, timeout=60)
        assert p.returncode == 0, (p.stdout[-300:], p.stderr[-2000:])
        kv = dict(l.split(b"=", 1) for l in p.stdout.splitlines())
        if int(kv[b"rc"]):
            return int(kv[b"rc"]), int(kv[b"line"]), kv[b"why"].decode()
        u = lambda k: np.array([int(x) for x in kv[k].split(b",") if x], np.uint64)
        return dict(text=bytes.fromhex(kv[b"text"].decode()), docs=bytes.fromhex(kv[b"docs"].decode()).decode(), pos=u(b"pos"), first=u(b"first"), val=u(b"val"),
                    skipped=dict(zip(MB.SKIPS, (int(x) for x in kv[b"skipped"].split(b",")))))
    return run


def agree(got, want):
    assert isinstance(got, dict), got
    assert got["text"] == bytes(want["text"])
    assert got["docs"] == "".join(f"{n} {s}\n" for n, s in zip(want["names"], want["starts"]))
    for k in ("pos", "first", "val"):
        assert (got[k] == want[k]).all() and len(got[k]) == len(want[k]), k
    assert got["skipped"] == want["skipped"]
    assert MB.records_ok(got["pos"], got["first"], len(got["text"]), 64)


def files(tmp_path, body, samples="s1\ts2", fa=FA, gz=False, name="x"):
    f = tmp_path / (name + ".fa")
    f.write_text(fa)
    v = tmp_path / (name + (".vcf.gz" if gz else ".vcf"))
    data = (HDR + samples + "\n" + body).encode() if isinstance(body, str) else body
    v.write_bytes(gzip.compress(data) if gz else data)
    return f, v


def test_the_fixture(check):
    fa, vcf = os.path.join(DATA, "small.fa"), os.path.join(DATA, "small.fa.vcf.gz")
    want = MB.vcf_text(fa, vcf, None, 10)
    got = check(fa, vcf)
    agree(got, want)
    assert want["names"] == ["ref", "sample0.1.ref", "sample0.2.ref"] and len(want["pos"]) == 30
    # the 0|0 site still gives allele-0 records in all three documents
    zero = [int(v) & 0xFFFFFFFFFFFF for v in want["val"] if int(v) >> 60 == 0]
    assert any(zero.count(p) == 3 for p in set(zero))


BODY = ("chr1\t1\t.\tA\tC\t.\t.\t.\tGT\t1|0\t0|1\n"            # contig position 0
        "chr1\t9\t.\ta\tg,T\t.\t.\t.\tGT:DP\t2|1:7\t.|2:3\n"    # w - 2, multi-allelic, lower case, a '.' allele
        "chr1\t10\t.\tC\tT\t.\t.\t.\tGT\t0|0\t1|1\n"           # w - 1
        "chr1\t30\t.\tC\tA\t.\t.\t.\tDP:GT\t5:1/1\t2:0|1\n"    # the last base; '/' between equal alleles
        "chr2\t20\t.\tC\tG\t.\t.\t.\tGT\t1\t0|1\n"             # the last base of the last contig; s1 haploid on chr2
        "chr2\t3\t.\tG\tA\t.\t.\t.\tGT\t.\t1|0\n")             # unsorted input


def test_two_contigs_two_samples_and_the_window_clip(check, tmp_path):
    for gz in (False, True):
        fa, vcf = files(tmp_path, BODY, gz=gz)
        for w in (10, 1, 64):
            want = MB.vcf_text(fa, vcf, None, w)
            agree(check(fa, vcf, w), want)
    assert want["names"] == ["chr1", "chr2", "s1.1.chr1", "s1.1.chr2", "s1.2.chr1", "s2.1.chr1", "s2.1.chr2", "s2.2.chr1", "s2.2.chr2"]
    w10 = MB.vcf_text(fa, vcf, None, 10)
    assert {int(p - f) for p, f in zip(w10["pos"], w10["first"])} >= {0, 8, 9}
    alleles = {int(v) >> 60 for v in w10["val"]}
    assert alleles == {0, 1, 2} and {(int(v) >> 48) & 0xFFF for v in w10["val"]} == {0, 1}
    t = bytes(w10["text"])
    s = w10["starts"][2]
    assert t[s] == ord("C") and t[s + 8] == ord("T") and t[w10["starts"][4] + 8] == ord("G")      # 2|1: the second ALT on haplotype 1, the first on 2


def test_sample_selection_and_order(check, tmp_path):
    fa, vcf = files(tmp_path, BODY)
    for sel in (["s2"], ["s1"], ["s2", "s1"], ["s1", "s2"], ["s2", "s2"]):
        want = MB.vcf_text(fa, vcf, sel, 10)
        agree(check(fa, vcf, 10, sel), want)
    both = MB.vcf_text(fa, vcf, ["s2", "s1"], 10)
    assert both["names"][2].startswith("s1.") and bytes(both["text"]) == bytes(MB.vcf_text(fa, vcf, None, 10)["text"])
    assert MB.vcf_text(fa, vcf, ["s2"], 10)["names"][2:] == ["s2.1.chr1", "s2.1.chr2", "s2.2.chr1", "s2.2.chr2"]


def test_crlf_and_no_final_newline(check, tmp_path):
    plain = MB.vcf_text(*files(tmp_path, BODY), None, 10)
    for name, data in (("crlf", (HDR + "s1\ts2\n" + BODY).replace("\n", "\r\n")), ("cut", (HDR + "s1\ts2\n" + BODY).rstrip("\n"))):
        fa, vcf = files(tmp_path, data.encode(), name=name)
        got = check(fa, vcf)
        agree(got, MB.vcf_text(fa, vcf, None, 10))
        assert got["text"] == bytes(plain["text"]) and (got["val"] == plain["val"]).all()


SKIPPED = {
    "indel": ("chr1\t5\t.\tAC\tA\t.\t.\t.\tGT\t0|1\t0|0\nchr1\t6\t.\tC\tCGG\t.\t.\t.\tGT\t0|1\t0|0\nchr1\t7\t.\tGT\tCA\t.\t.\t.\tGT\t0|1\t0|0\n", 3),
    "symbolic": ("chr1\t5\t.\tA\t<DEL>\t.\t.\t.\tGT\t0|1\t0|0\nchr1\t6\t.\tC\t*\t.\t.\t.\tGT\t0|1\t0|0\nchr1\t7\t.\tG\tN\t.\t.\t.\tGT\t0|1\t0|0\n"
                 "chr1\t8\t.\tT\tT]chr2:5]\t.\t.\t.\tGT\t0|1\t0|0\n", 4),
    "contig": ("chrX\t5\t.\tA\tC\t.\t.\t.\tGT\t0|1\t0|0\nchrX\t999\t.\tA\tC\t.\t.\t.\tGT\t0|1\t0|0\n", 2),
    "duplicate": ("chr1\t2\t.\tC\tG\t.\t.\t.\tGT\t1|1\t1|1\nchr1\t2\t.\tC\tA\t.\t.\t.\tGT\t1|1\t1|1\n", 1),
}


@pytest.mark.parametrize("kind", sorted(SKIPPED))
def test_skipped_sites_are_counted(check, tmp_path, kind):
    body, count = SKIPPED[kind]
    fa, vcf = files(tmp_path, "chr1\t1\t.\tA\tC\t.\t.\t.\tGT\t1|0\t0|1\n" + body)
    want = MB.vcf_text(fa, vcf, None, 10)
    assert want["skipped"] == {**dict.fromkeys(MB.SKIPS, 0), kind: count}
    got = check(fa, vcf)
    agree(got, want)
    if kind == "duplicate":      # the first is kept
        assert bytes(want["text"])[want["starts"][2] + 1] == ord("G")


REFUSED = {
    "no #CHROM line": (b"##fileformat=VCFv4.2\nchr1\t1\t.\tA\tC\t.\t.\t.\tGT\t1|0\t0|1\n", 2),
    "no #CHROM line at all": (b"##fileformat=VCFv4.2\n##x\n", 3),
    "nine columns": ((HDR.rstrip("\t") + "\n").encode(), 2),
    "a short record": ((HDR + "s1\ts2\nchr1\t1\t.\tA\tC\t.\t.\t.\tGT\t1|0\n").encode(), 3),
    "REF disagrees": ((HDR + "s1\ts2\nchr1\t1\t.\tA\tC\t.\t.\t.\tGT\t1|0\t0|1\nchr1\t2\t.\tG\tC\t.\t.\t.\tGT\t1|0\t0|1\n").encode(), 4),
    "POS 0": ((HDR + "s1\ts2\nchr1\t0\t.\tA\tC\t.\t.\t.\tGT\t1|0\t0|1\n").encode(), 3),
    "POS beyond the contig": ((HDR + "s1\ts2\nchr2\t21\t.\tA\tC\t.\t.\t.\tGT\t1|0\t0|1\n").encode(), 3),
    "unphased": ((HDR + "s1\ts2\nchr1\t1\t.\tA\tC\t.\t.\t.\tGT\t1|0\t0/1\n").encode(), 3),
    "ploidy changes": ((HDR + "s1\ts2\nchr1\t1\t.\tA\tC\t.\t.\t.\tGT\t1|0\t0|1\n\nchr1\t2\t.\tC\tG\t.\t.\t.\tGT\t1\t0|1\n").encode(), 5),
    "allele beyond the ALTs": ((HDR + "s1\ts2\nchr1\t1\t.\tA\tC\t.\t.\t.\tGT\t2|0\t0|1\n").encode(), 3),
    "no GT": ((HDR + "s1\ts2\nchr1\t1\t.\tA\tC\t.\t.\t.\tDP\t3\t4\n").encode(), 3),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_name_the_line(check, tmp_path, name):
    data, line = REFUSED[name]
    for gz in (False, True):
        fa, vcf = files(tmp_path, data, gz=gz)
        with pytest.raises(MB.VcfRefused) as e:
            MB.vcf_text(fa, vcf, None, 10)
        assert e.value.line == line
        rc, got_line, why = check(fa, vcf)
        assert (rc, got_line) == (EFORMAT, line) and f"line {line} " in why, (name, why)


def test_an_absent_sample_and_too_many_contigs(check, tmp_path):
    fa, vcf = files(tmp_path, BODY)
    rc, line, why = check(fa, vcf, 10, ["s1", "nobody"])
    assert (rc, line) == (EFORMAT, 2) and "nobody" in why
    with pytest.raises(MB.VcfRefused):
        MB.vcf_text(fa, vcf, ["nobody"], 10)
    many = "".join(f">c{k}\nAC\n" for k in range(4097))
    fa2, vcf2 = files(tmp_path, "", fa=many, name="many")
    rc, line, why = check(fa2, vcf2)
    assert (rc, line) == (EFORMAT, 0) and "4096" in why
    fa3, vcf3 = files(tmp_path, "c4095\t1\t.\tA\tC\t.\t.\t.\tGT\t1|0\t0|1\n", fa=many[:many.index(">c4096")], name="most")
    got = check(fa3, vcf3)
    agree(got, MB.vcf_text(fa3, vcf3, None, 10))
    assert {(int(v) >> 48) & 0xFFF for v in got["val"]} == {4095}
