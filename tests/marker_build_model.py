"""The rule of the marker build (include/rbg.h, rowbowt_amd/csrc/mk_build.hip, rbg_vcf.hpp) restated in numpy and plain Python: no device, no torch.

A site record is (pos, first, val): the row i with p = sa[i] carries the values of every record with first <= p <= pos, ascending; a covered row continues
the run of the covered row before it only if the two are adjacent, both carry exactly one value, and it is the same one; a run's values are those of its
first row.  marker_runs applies that through an inverse suffix array, which the device pass never builds.

vcf_text is the model of rbg_vcf.hpp: the reference's contigs, then per selected sample and haplotype every contig with that haplotype's alleles applied,
and one record per document and accepted site."""
import gzip
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "data")
U64 = np.uint64


def marker_value(allele, contig, refpos):
    return (int(allele) << 60) | (int(contig) << 48) | int(refpos)


def records(docs, w):
    """docs: [(start of the document in the text, [(offset in the document, value), ...])] -> (pos, first, val) uint64, sorted by pos"""
    out = []
    for start, sites in docs:
        for off, val in sites:
            out.append((start + off, max(start, start + off - w + 1), val))
    out.sort()
    a = np.array(out, dtype=object).reshape(-1, 3)
    return tuple(np.array([int(x) for x in a[:, k]], dtype=U64) for k in range(3))


def records_ok(pos, first, n, w):
    """the input rule of the device pass"""
    pos, first = np.asarray(pos, U64).astype(object), np.asarray(first, U64).astype(object)
    if not 1 <= w <= 64:
        return False
    for r in range(len(pos)):
        if not (first[r] <= pos[r] < n and pos[r] - first[r] < w):
            return False
        if r and not (pos[r - 1] < pos[r] and first[r - 1] <= first[r]):
            return False
    return True


def marker_runs(sa, pos, first, val):
    """-> (run_start, run_end, mk_off, mk_vals), uint64: the arguments of rbg_set_markers"""
    sa = np.asarray(sa).astype(np.int64)
    n = len(sa)
    pos, first, val = (np.asarray(a, U64) for a in (pos, first, val))
    if len(pos) == 0:
        z = np.zeros(0, U64)
        return z, z.copy(), np.zeros(1, U64), z.copy()
    isa = np.empty(n, np.int64)
    isa[sa] = np.arange(n)
    span = (pos - first).astype(np.int64) + 1
    rec = np.repeat(np.arange(len(pos)), span)
    p = np.repeat(first.astype(np.int64), span) + (np.arange(int(span.sum())) - np.repeat(np.cumsum(span) - span, span))
    rows, vals = isa[p], val[rec]
    order = np.lexsort((vals, rows))
    rows, vals = rows[order], vals[order]
    urows, start, counts = np.unique(rows, return_index=True, return_counts=True)
    v0 = vals[start]
    cont = np.zeros(len(urows), bool)
    cont[1:] = (counts[1:] == 1) & (counts[:-1] == 1) & (urows[1:] == urows[:-1] + 1) & (v0[1:] == v0[:-1])
    head = np.flatnonzero(~cont)
    last = np.append(head[1:] - 1, len(urows) - 1)
    cnt = counts[head]
    mk_off = np.zeros(len(head) + 1, np.int64)
    mk_off[1:] = np.cumsum(cnt)
    src = np.repeat(start[head], cnt) + (np.arange(int(mk_off[-1])) - np.repeat(mk_off[:-1], cnt))
    return urows[head].astype(U64), urows[last].astype(U64), mk_off.astype(U64), vals[src].astype(U64)


def covered_rows(sa, pos, first):
    """the rows that carry a value, ascending"""
    sa = np.asarray(sa).astype(np.int64)
    cov = np.zeros(len(sa) + 1, np.int64)
    np.add.at(cov, np.asarray(first, U64).astype(np.int64), 1)
    np.add.at(cov, np.asarray(pos, U64).astype(np.int64) + 1, -1)
    return np.flatnonzero(np.cumsum(cov)[:-1][sa] > 0)


# ---- FASTA and VCF, as rbg_fasta_text.hpp and rbg_vcf.hpp read them ------------------------------------------------------------------------------------
def read_fasta(path):
    """[(name, upper-cased sequence bytes)]"""
    raw = gzip.open(path, "rb").read() if open(path, "rb").read(2) == b"\x1f\x8b" else open(path, "rb").read()
    out = []
    for line in raw.replace(b"\r", b"").split(b"\n"):
        if line.startswith(b">"):
            out.append([line[1:].split()[0].decode(), bytearray()])
        elif out:
            out[-1][1] += line.upper()
    return [(n, bytes(s)) for n, s in out]


class VcfRefused(Exception):
    def __init__(self, line, why):
        super().__init__(f"line {line}: {why}")
        self.line = line


SKIPS = ("indel", "symbolic", "contig", "duplicate")


def vcf_text(fasta, vcf, samples=None, w=10):
    """-> dict(text, names, starts, pos, first, val, skipped {kind: count}); VcfRefused(line number) where rbg_vcf.hpp returns RBG_EFORMAT"""
    contigs = read_fasta(fasta)
    if len(contigs) > 4096:
        raise VcfRefused(0, "more than 4096 contigs")
    cidx = {n: k for k, (n, _s) in enumerate(contigs)}
    raw = open(vcf, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    lines = raw.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    cols, chosen = None, None
    skipped = dict.fromkeys(SKIPS, 0)
    sites = [dict() for _ in contigs]          # contig -> {pos0: per chosen sample the allele list}
    ploidy = {}                                # (sample column, contig) -> ploidy
    for ln, line in enumerate(lines, 1):
        line = line.rstrip(b"\r").decode("latin-1")
        if line.startswith("##") or not line:
            continue
        if line.startswith("#CHROM"):
            cols = line.split("\t")
            if len(cols) < 10:
                raise VcfRefused(ln, "fewer than 10 columns")
            names = cols[9:]
            if samples is None:
                chosen = list(range(len(names)))
            else:
                for s in samples:
                    if s not in names:
                        raise VcfRefused(ln, f"sample {s} is absent")
                chosen = sorted({names.index(s) for s in samples})   # VCF column order
            continue
        if line.startswith("#"):
            continue
        if cols is None:
            raise VcfRefused(ln, "no #CHROM line")
        f = line.split("\t")
        if len(f) < 10 or len(f) != len(cols):
            raise VcfRefused(ln, "fewer than 10 columns")
        chrom, ref, alts = f[0], f[3].upper(), f[4].upper().split(",")
        if chrom not in cidx:
            skipped["contig"] += 1
            continue
        c = cidx[chrom]
        seq = contigs[c][1]
        if not f[1].isdigit() or int(f[1]) == 0 or int(f[1]) > len(seq):
            raise VcfRefused(ln, "POS outside the contig")
        p0 = int(f[1]) - 1
        if any(a.startswith("<") or a == "*" or "[" in a or "]" in a for a in alts):
            skipped["symbolic"] += 1
            continue
        if len(ref) != 1 or any(len(a) != 1 for a in alts):
            skipped["indel"] += 1
            continue
        if ref not in "ACGT" or any(a not in "ACGT" for a in alts) or len(alts) > 15:
            skipped["symbolic"] += 1
            continue
        if seq[p0:p0 + 1].decode() != ref:
            raise VcfRefused(ln, "REF disagrees with the FASTA")
        if p0 in sites[c]:
            skipped["duplicate"] += 1
            continue
        gi = f[8].split(":").index("GT") if "GT" in f[8].split(":") else None
        if gi is None:
            raise VcfRefused(ln, "no GT")
        per = []
        for s in chosen:
            sf = f[9 + s].split(":")
            if gi >= len(sf):
                raise VcfRefused(ln, "no GT for the sample")
            gt = sf[gi]
            parts = gt.replace("/", "|").split("|")
            al = []
            for a in parts:
                if a == ".":
                    al.append(0)
                elif a.isdigit() and int(a) <= len(alts):
                    al.append(int(a))
                else:
                    raise VcfRefused(ln, "bad GT")
            if "/" in gt and len(set(al)) > 1:
                raise VcfRefused(ln, "unphased heterozygous GT")
            if ploidy.setdefault((s, c), len(al)) != len(al):
                raise VcfRefused(ln, "ploidy changes")
            per.append(al)
        sites[c][p0] = (ref, alts, per)
    if cols is None:
        raise VcfRefused(len(lines) + 1, "no #CHROM line")
    names, seqs, recs = [], [], []             # recs: per document [(offset, value)]
    for c, (n, s) in enumerate(contigs):
        names.append(n)
        seqs.append(s)
        recs.append([(p0, marker_value(0, c, p0)) for p0 in sorted(sites[c])])
    for k, s in enumerate(chosen):
        nhap = max([ploidy.get((s, c), 0) for c in range(len(contigs))] + [0])
        for h in range(nhap):
            for c, (n, seq) in enumerate(contigs):
                if ploidy.get((s, c), nhap) <= h:
                    continue
                b = bytearray(seq)
                r = []
                for p0 in sorted(sites[c]):
                    ref, alts, per = sites[c][p0]
                    a = per[k][h]
                    if a:
                        b[p0] = ord(alts[a - 1])
                    r.append((p0, marker_value(a, c, p0)))
                names.append(f"{cols[9 + s]}.{h + 1}.{n}")
                seqs.append(bytes(b))
                recs.append(r)
    starts = np.cumsum([0] + [len(s) + 1 for s in seqs])[:-1].tolist()
    text = b"#".join(seqs) + b"\x01"
    pos, first, val = records(list(zip(starts, recs)), w)
    return dict(text=np.frombuffer(text, np.uint8).copy(), names=names, starts=starts, pos=pos, first=first, val=val, skipped=skipped)


def fixture_layout(w=10):
    """the text small.fa.{rbwt,mab} were built over: ref + 10 x A + hap1 + 10 x A + hap2 + 10 x A + 0x01, with its site records"""
    v = vcf_text(os.path.join(DATA, "small.fa"), os.path.join(DATA, "small.fa.vcf.gz"), None, w)
    docs = bytes(v["text"][:-1]).split(b"#")
    assert len(docs) == 3 and all(len(d) == 10000 for d in docs)
    text = b"".join(d + b"A" * 10 for d in docs) + b"\x01"
    starts = [0, 10010, 20020]
    per_doc = [[(int(p) - s, int(x)) for p, x in zip(v["pos"], v["val"]) if s <= int(p) < s + 10000] for s in v["starts"]]
    pos, first, val = records(list(zip(starts, per_doc)), w)
    return dict(text=np.frombuffer(text, np.uint8).copy(), starts=starts, pos=pos, first=first, val=val)
