"""Test infrastructure: the marker tally's PER-READ mode as a function of rb_markers' stdout (the specification of RBG_TALLY_PER_READ and
RBG_TALLY_DROP_SITE_CONFLICTS, include/rbg.h).  The lines are grouped by read name, so the caller gives every read a unique name first (its
index, say) and calls rb_markers_model.expected_stdout ONCE for the whole batch (the heuristic's coin stream runs across reads).

One read, its lines in print order: for each distinct marker m on them, the line carrying m with the greatest query_len -- the earliest on a tie --
adds 1 to n_fwd[m] or n_rev[m] by its strand and its query_len to len_sum[m].  With drop_site_conflicts, a read whose lines carry two or more
alleles of one site (the marker's bits 0-59) adds nothing for any marker of that site."""
from tally_model import M64, make_marker, sorted_entries

SITE = (1 << 60) - 1


def parse_lines(text):
    """stdout -> {name: [(strand, query_len, [markers])]} with the reads in order of first appearance and each read's lines in print order"""
    reads = {}
    for line in text.splitlines():
        f = line.split(" ")
        assert len(f) >= 6 and f[2] in "+-", line
        ms = []
        if f[5:] != ["."]:
            for tok in f[5:]:
                seq, pos, allele = (int(x) for x in tok.split("/"))
                ms.append(make_marker(seq, pos, allele))
        reads.setdefault(f[0], []).append((f[2], int(f[4]), ms))
    return reads


def read_counts(text, drop_site_conflicts=False):
    """what rbg_tally_read_info reports besides the number of reads: {"elements_seen", "added", "lost", "site_dropped"}; an element is one marker on
    one line.  Every element of a conflicted site is site_dropped; of the others, all but the winning one per (read, marker) are lost."""
    seen = added = lost = dropped = 0
    for lines in parse_lines(text).values():
        alleles = {}
        for _, _, ms in lines:
            for m in ms:
                alleles.setdefault(m & SITE, set()).add(m >> 60)
        winners = set()
        for _, _, ms in lines:
            for m in ms:
                seen += 1
                if drop_site_conflicts and len(alleles[m & SITE]) > 1:
                    dropped += 1
                elif m in winners:
                    lost += 1
                else:
                    winners.add(m)
                    added += 1
    return dict(elements_seen=seen, added=added, lost=lost, site_dropped=dropped)


def tally_reads_from_stdout(text, drop_site_conflicts=False):
    """rb_markers' stdout (unique read names) -> ({marker: (n_fwd, n_rev, len_sum)}, the sorted entry list): tally_model.tally_from_stdout's shape"""
    table = {}
    for lines in parse_lines(text).values():
        best, alleles = {}, {}                       # marker -> (query_len, -line index) of its winning line
        for i, (_, qlen, ms) in enumerate(lines):
            for m in ms:
                alleles.setdefault(m & SITE, set()).add(m >> 60)
                if m not in best or (qlen, -i) > best[m]:
                    best[m] = (qlen, -i)
        for m, (qlen, neg_i) in best.items():
            if drop_site_conflicts and len(alleles[m & SITE]) > 1:
                continue
            strand = lines[-neg_i][0]
            nf, nr, ls = table.get(m, (0, 0, 0))
            table[m] = (nf + (strand == "+"), nr + (strand == "-"), (ls + qlen) & M64)
    return table, sorted_entries(table)
