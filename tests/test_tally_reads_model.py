"""CPU-only checks of the tally's per-read mode: the rule itself on hand-written lines (tests/tally_reads_model.py is the specification of
RBG_TALLY_PER_READ / RBG_TALLY_DROP_SITE_CONFLICTS), the numbers that motivated it on the toy read set, rb_markers' flag checks and the exports."""
import os
import re

import pytest

import orc
import rb_markers_model as RM
import rowbowt_amd as ra
import tally_model as TM
import tally_reads_model as TR
import toy_read_set as TS
from gpu_common import _run_rb_markers
from lmem_model import LmemAsGreedy
from rowbowt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rbg_markers_tally_reads", "rbg_tally_add_reads_tmp_bytes", "rbg_tally_add_reads_dev", "rbg_tally_read_info")
mk = TM.make_marker


def _both(text):
    return TR.tally_reads_from_stdout(text)[0], TR.tally_reads_from_stdout(text, drop_site_conflicts=True)[0]


# ---- 1. the rule on hand-written lines ---------------------------------------------------------------------------------------------------

def test_tie_goes_to_the_earliest_line():
    text = "r 3 - 0 33 1/5/0\nr 3 + 7 33 1/5/0\nr 3 + 9 20 1/5/0\n"
    plain, sites = _both(text)
    assert plain == sites == {mk(1, 5, 0): (0, 1, 33)}
    assert TM.tally_from_stdout(text)[0] == {mk(1, 5, 0): (2, 1, 86)}
    assert TR.read_counts(text) == dict(elements_seen=3, added=1, lost=2, site_dropped=0)


def test_greatest_query_len_wins_across_strands():
    text = "r 3 + 0 7 1/5/0 1/9/2\nr 3 - 7 33 1/5/0\nq 1 + 0 8 1/5/0\n"      # read q is another read: it counts on its own
    plain, sites = _both(text)
    assert plain == sites == {mk(1, 5, 0): (1, 1, 41), mk(1, 9, 2): (1, 0, 7)}


def test_both_alleles_on_one_line():
    text = "r 9 + 0 20 2/100/0 2/100/1 2/101/1\n"
    plain, sites = _both(text)
    assert plain == {mk(2, 100, 0): (1, 0, 20), mk(2, 100, 1): (1, 0, 20), mk(2, 101, 1): (1, 0, 20)}
    assert sites == {mk(2, 101, 1): (1, 0, 20)}
    assert TR.read_counts(text, True) == dict(elements_seen=3, added=1, lost=0, site_dropped=2)


def test_both_alleles_over_two_lines():
    text = "r 9 + 0 20 2/100/0\nr 9 - 30 25 2/100/1 2/101/1\nr 9 - 60 9 2/100/1\ns 1 + 0 12 2/100/1\n"
    plain, sites = _both(text)
    assert plain == {mk(2, 100, 0): (1, 0, 20), mk(2, 100, 1): (1, 1, 37), mk(2, 101, 1): (0, 1, 25)}
    assert sites == {mk(2, 100, 1): (1, 0, 12), mk(2, 101, 1): (0, 1, 25)}          # read s carries one allele only and still counts
    assert TR.read_counts(text, True) == dict(elements_seen=5, added=2, lost=0, site_dropped=3)   # every copy of a dropped element counts
    assert TR.read_counts(text, False) == dict(elements_seen=5, added=4, lost=1, site_dropped=0)


def test_dot_line_and_marker_all_ones():
    top = f"{0xFFF}/{2**48 - 1}/15"
    other = f"{0xFFF}/{2**48 - 1}/3"
    text = f"r 1 + 0 10 .\nr 1 - 0 11 {top}\nr 1 - 5 11 {top}\nq 1 + 0 5 {other} {top}\n"
    plain, sites = _both(text)
    assert plain == {TM.M64: (1, 1, 16), mk(0xFFF, 2**48 - 1, 3): (1, 0, 5)}
    assert sites == {TM.M64: (0, 1, 11)}                                             # 2^64 - 1 is allele 15 of its site, like any other marker
    assert TR.tally_reads_from_stdout("r 1 + 0 10 .\n") == ({}, [])


def test_len_sum_wraps():
    text = f"a 1 + 0 {2**63} 1/1/1\nb 1 - 0 {2**63 + 5} 1/1/1\n"
    assert TR.tally_reads_from_stdout(text)[0] == {mk(1, 1, 1): (1, 1, 5)}


# ---- 2. the toy read set: the numbers behind the mode --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def toy(data_dir):
    o = orc.Oracle.load(os.path.join(data_dir, "small.fa"), orc.SA | orc.MA)
    yield o, TS.renamed(TS.toy_reads(data_dir))
    o.close()


def _figures(text):
    """(elements on printed lines, distinct (read, marker) pairs, reads with a marker on >= 2 lines, ... on lines of both strands, reads whose
    lines carry two alleles of one site)"""
    reads = TR.parse_lines(text)
    elements = sum(len(ms) for lines in reads.values() for _, _, ms in lines)
    pairs = dup = both = two = 0
    for lines in reads.values():
        on = {}
        for strand, _, ms in lines:
            for m in ms:
                on.setdefault(m, []).append(strand)
        pairs += len(on)
        dup += any(len(v) > 1 for v in on.values())
        both += any(len(set(v)) > 1 for v in on.values())
        sites = {}
        for m in on:
            sites.setdefault(m & TR.SITE, set()).add(m >> 60)
        two += any(len(a) > 1 for a in sites.values())
    return elements, pairs, dup, both, two


CASES = [("default", dict(), False, (19, 19, 0, 0, 0)), ("wsize5", dict(wsize=5), False, (880, 811, 45, 16, 155)),
         ("ftab", dict(wsize=8, ftab_k=6), False, (74, 73, 1, 0, 7)), ("lmem", dict(wsize=8, ftab_k=6), True, (50, 13, 3, 0, 1))]


@pytest.mark.parametrize("name,kw,lmem,want", CASES, ids=[c[0] for c in CASES])
def test_toy_figures(toy, name, kw, lmem, want):
    o, recs = toy
    if lmem:
        recs, o = TS.dozen(recs), LmemAsGreedy(o)
    elif kw.get("ftab_k"):
        recs = [r for r in recs if len(r[1]) >= 6]
    text = RM.expected_stdout(o, recs, **kw)
    assert _figures(text) == want
    line = TM.tally_from_stdout(text)
    plain, sites = TR.tally_reads_from_stdout(text), TR.tally_reads_from_stdout(text, True)
    if want[0] == want[1]:
        assert plain == line                                    # no duplicates: per-read mode IS line mode
    else:
        assert plain != line
    assert (sites == plain) == (want[4] == 0)
    for a, b in ((plain, line), (sites, plain)):                # field by field at most the coarser mode's counts
        assert set(a[0]) <= set(b[0])
        for m, (nf, nr, _) in a[0].items():
            assert nf <= b[0][m][0] and nr <= b[0][m][1]
    c, cs = TR.read_counts(text), TR.read_counts(text, True)
    assert c["elements_seen"] == want[0] and c["added"] == want[1] and c["lost"] == want[0] - want[1] and c["site_dropped"] == 0
    for cc, t in ((c, plain), (cs, sites)):
        assert cc["elements_seen"] == cc["added"] + cc["lost"] + cc["site_dropped"]
        assert cc["added"] == sum(nf + nr for _, nf, nr, _ in t[1])


# ---- 3. the tool's flag checks and the exports ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args", [["--tally-per-read"], ["--tally-drop-conflicts"], ["--tally-per-read", "--tally-drop-conflicts"],
                                  ["--tally", "OUT", "--tally-drop-conflicts"], ["--heuristic", "--tally-per-read"]], ids=" ".join)
def test_cli_flag_misuse(args, tmp_path):
    """each exits 1 with a message before anything is loaded: the index prefix does not exist, and no device is asked for"""
    out = tmp_path / "out.tsv"
    args = [str(out) if a == "OUT" else a for a in args]
    rc, stdout, err = _run_rb_markers(args + [str(tmp_path / "no_such_index"), str(tmp_path / "no_such.fq")])
    assert rc == 1 and stdout == "" and "--tally" in err and "rb_markers:" in err
    assert not out.exists()


def test_exports_and_header():
    L = ra.lib()
    hdr = open(os.path.join(ROOT, "include", "rbg.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert re.search(r"#define\s+RBG_TALLY_PER_READ\s+1u", hdr) and re.search(r"#define\s+RBG_TALLY_DROP_SITE_CONFLICTS\s+2u", hdr)
    assert (capi.TALLY_PER_READ, capi.TALLY_DROP_SITE_CONFLICTS) == (1, 2) and capi.ABI_VERSION == 3
    assert L.rbg_tally_add_reads_tmp_bytes(10, 1000) >= L.rbg_tally_add_tmp_bytes(1000) + 8 * 1000
    assert L.rbg_tally_read_info(None, None) == -4
    assert L.rbg_tally_add_reads_dev(None, None, 0, None, 0, None, 0, 0, None, 0, None) == -4
