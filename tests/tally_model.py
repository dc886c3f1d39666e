"""Test infrastructure: the marker tally as a function of rb_markers' stdout.  For every printed line and every marker on it, n_fwd or n_rev
(by the line's strand) goes up by one and len_sum by the line's query_len; a line with " ." adds nothing.  The marker value is rebuilt from
<seq>/<pos>/<allele> with the field layout of rb_markers_model / golden_values (allele 60-63, sequence 48-59, position 0-47)."""
M64 = 2**64 - 1


def make_marker(seq, pos, allele):
    return ((allele & 0xF) << 60) | ((seq & 0xFFF) << 48) | (pos & ((1 << 48) - 1))


def rotl4(m):
    return ((m << 4) | (m >> 60)) & M64


def sorted_entries(table):
    """{marker: (n_fwd, n_rev, len_sum)} -> [(marker, n_fwd, n_rev, len_sum)] in export order: ascending rotl64(marker, 4), entries without counts left out"""
    return [(m,) + tuple(v) for m, v in sorted(table.items(), key=lambda kv: rotl4(kv[0])) if v[0] + v[1] > 0]


def tally_from_stdout(text):
    """rb_markers' stdout -> ({marker: (n_fwd, n_rev, len_sum)}, the sorted entry list).  A line is
    "<name> <range_size> <+|-> <query_start> <query_len>" then " ." or one " <seq>/<pos>/<allele>" per marker (names hold no blank)."""
    table = {}
    for line in text.splitlines():
        f = line.split(" ")
        assert len(f) >= 6 and f[2] in "+-", line
        if f[5:] == ["."]:
            continue
        qlen = int(f[4])
        for tok in f[5:]:
            seq, pos, allele = (int(x) for x in tok.split("/"))
            m = make_marker(seq, pos, allele)
            nf, nr, ls = table.get(m, (0, 0, 0))
            table[m] = (nf + (f[2] == "+"), nr + (f[2] == "-"), (ls + qlen) & M64)
    return table, sorted_entries(table)


def add_tables(*tables):
    out = {}
    for t in tables:
        for m, (nf, nr, ls) in t.items():
            a = out.get(m, (0, 0, 0))
            out[m] = (a[0] + nf, a[1] + nr, (a[2] + ls) & M64)
    return out


def entries_tsv(entries):
    """the file `rb_markers --tally` writes"""
    return "".join(f"{(m >> 48) & 0xFFF}\t{m & ((1 << 48) - 1)}\t{m >> 60}\t{nf}\t{nr}\t{ls}\n" for m, nf, nr, ls in entries)


def entries_from_tsv(text):
    out = []
    for line in text.splitlines():
        seq, pos, allele, nf, nr, ls = (int(x) for x in line.split("\t"))
        out.append((make_marker(seq, pos, allele), nf, nr, ls))
    return out
