"""The ISA sample's model (tests/isa_model.py: builder, directory, lookup, ISA, extract) against the text itself (text_ref.TextRef) on two texts: the
2 051-symbol pangenome of the FL tests, whose only byte that is no base is the terminator, and a text built by hand with documents separated by '#', a run of
five N inside one document and a document that starts with N."""
import pytest

import isa_model as IM
from text_ref import TextRef


@pytest.fixture(scope="module", params=["synth", "hand"])
def case(request):
    T = IM.synth_text() if request.param == "synth" else IM.hand_text()
    ref = TextRef(T.text, T.sa)
    return request.param, T, ref, T.model()


def test_the_hand_text_has_what_it_is_for():
    T = IM.hand_text()
    M = T.model()
    assert T.tb.count(b"#") == 2 and b"NNNNN" in T.tb and T.tb[T.doc_starts[1]] == ord("N") and T.tb[T.doc_starts[1] - 1] == ord("#")
    assert M.longest_other_run >= 3 and M.second_kind >= 2                 # the BWT has a non-base run of three or more: the second kind exists
    assert M.samples == len(T.heads) + M.second_kind
    # without the second kind at least one position's walk-in meets a row without a base
    bare = T.model(second_kind=False)
    assert bare.samples == len(T.heads)
    stuck = [p for p in range(T.n) if bare.isa(p) is None]
    assert stuck and all(M.isa(p) is not None for p in stuck)


def test_samples_are_suffix_array_pairs(case):
    name, T, ref, M = case
    assert all(int(ref.sa[r]) == p for p, r in zip(M.tpos, M.row))
    assert M.tpos[0] == 0 and M.tpos == sorted(M.tpos)
    # a sample right behind every byte that is no base: none between a position and the sample before it
    for s, c in enumerate(T.tb):
        if c not in IM.ACGT:
            assert (s + 1) % T.n in M.tpos
    assert M.bytes(4) == M.samples * 8 + ((T.n >> M.shift) + 2) * 4 and M.bytes(8) == 2 * M.bytes(4)
    assert (M.samples << M.shift) <= T.n < (M.samples << (M.shift + 1))
    assert M.max_gap == max(b - a for a, b in zip(M.tpos, M.tpos[1:] + [T.n]))


def test_isa_at_every_position(case):
    name, T, ref, M = case
    for p in range(T.n):
        q, row = M.lookup(p)
        assert q == max(t for t in M.tpos if t <= p) and p - q < M.max_gap
        assert M.isa(p) == int(ref.isa[p]), p


def test_extract_at_every_position_and_length(case):
    name, T, ref, M = case
    for p in range(T.n):
        row = M.isa(p)
        for length in IM.LENS:
            want = IM.expected(T.tb, p, length)
            assert M.extract_from(row, length) == want, (p, length)
            assert len(want[0]) == length and want[0][want[1]:] == bytes(length - want[1])
    ends = {T.tb[p + IM.expected(T.tb, p, 70)[1]] for p in range(T.n) if IM.expected(T.tb, p, 70)[1] < 70 and p + IM.expected(T.tb, p, 70)[1] < T.n}
    assert ends == ({1} if name == "synth" else {1, ord("#"), ord("N")})
