"""tests/arena.py on CPU tensors: a carve has the size, alignment and skew asked for; a clean arena passes; every planted single-byte write -- just
below a carve, just behind it, at the guard's far end, inside a declared-untouched range, into a snapshotted input -- is caught and named with its
region, side and byte offset.  (The GPU side of the same checks: tests/test_gpu_footprint.py.)"""
import numpy as np
import pytest
import torch

from arena import Arena, ArenaError, GUARD, PATTERN, default_skew


def _arena():
    A = Arena(1 << 14)
    A.carve("in", 40, 8)
    A.carve("locs", 8 * 13, 8)
    A.carve("recs", 56 * 3, 4)
    A.carve("ws", 1000, 256)
    A.carve("seqs", 48, 16)
    return A


def _poke(A, at, value=0x5A):
    A.buf[at] = value


@pytest.mark.parametrize("align", [1, 4, 8, 16, 32, 64, 256])
@pytest.mark.parametrize("nbytes", [0, 1, 7, 64, 1001])
def test_carve_has_the_size_alignment_and_skew_asked_for(align, nbytes):
    A = Arena(1 << 13)
    A.carve("first", 3, 1)
    r = A.carve("r", nbytes, align)
    after = A.carve("after", 5, 1, skew=63)
    assert r.nbytes == nbytes and r.u8.numel() == nbytes and r.end - r.begin == nbytes
    skew = default_skew(align)
    assert skew == (align if align < 64 else 0)
    assert r.data_ptr() % 64 == skew and r.data_ptr() % align == 0
    if align < 64:
        assert r.data_ptr() % (2 * align) == align     # at the minimum alignment and no better, off every 64-byte line
    if nbytes:
        assert r.u8.data_ptr() == r.data_ptr()
    assert r.begin - A["first"].end >= GUARD and after.begin - r.end >= GUARD and A.buf.numel() - after.end >= GUARD
    assert after.data_ptr() % 64 == 63
    assert bool((A.buf == PATTERN).all())
    A.check()


@pytest.mark.parametrize("skew", [8, 24, 56])
def test_explicit_skew_and_typed_views(skew):
    A = Arena(1 << 12)
    r = A.carve("locs", 8 * 9, 8, skew=skew)
    assert r.data_ptr() % 64 == skew
    v = r.view(torch.int64)
    assert v.numel() == 9 and v.data_ptr() == r.data_ptr()
    v.fill_(-7)
    assert (r.numpy(np.int64) == -7).all()
    A.check()                                   # writing a region's own bytes is no fault
    r.fill_from(np.arange(9, dtype=np.uint64))
    assert r.numpy(np.uint64).tolist() == list(range(9))
    with pytest.raises(ArenaError):
        r.fill_from(np.arange(8, dtype=np.uint64))
    with pytest.raises(ArenaError):
        A.carve("bad", 8, 8, skew=4)            # no multiple of the alignment
    with pytest.raises(ArenaError):
        A.carve("bad", 8, 256, skew=64)
    with pytest.raises(ArenaError):
        A.carve("locs", 8, 8)                   # a name is carved once
    with pytest.raises(ArenaError):
        A.carve("huge", 1 << 12, 8)


def test_clean_arena_passes():
    A = _arena()
    for r in A.regions:
        r.fill(0x11)                            # every region written to its last byte
    A.snapshot("in")
    A.check()
    A.check_untouched("locs", [])
    A.assert_unchanged("in")
    assert A.guard_faults() == []


@pytest.mark.parametrize("name", ["in", "locs", "recs", "ws", "seqs"])
@pytest.mark.parametrize("where,side,off", [("start-1", "before", 1), ("end", "after", 0)])
def test_write_next_to_a_carve_is_caught_and_named(name, where, side, off):
    A = _arena()
    r = A[name]
    _poke(A, r.begin - 1 if where == "start-1" else r.end)
    assert A.guard_faults() == [(name, side, off, 0x5A)]
    with pytest.raises(ArenaError) as ei:
        A.check()
    assert f"{name}: byte {off} {side} the region" in str(ei.value) and "0x5A" in str(ei.value)


def test_write_at_the_guards_far_end_is_caught():
    A = _arena()
    first, last = A.regions[0], A.regions[-1]
    _poke(A, first.begin - GUARD)
    _poke(A, last.end + GUARD - 1)
    assert A.guard_faults() == [("in", "before", GUARD, 0x5A), ("seqs", "after", GUARD - 1, 0x5A)]
    # between two carves the nearer one names the byte
    A2 = _arena()
    a, b = A2["locs"], A2["recs"]
    _poke(A2, b.begin - 3)
    _poke(A2, a.end + 2)
    assert A2.guard_faults() == [("locs", "after", 2, 0x5A), ("recs", "before", 3, 0x5A)]
    with pytest.raises(ArenaError) as ei:
        A2.check()
    assert "2 guard byte(s)" in str(ei.value)


def test_write_inside_a_declared_untouched_range_is_caught():
    A = _arena()
    r = A["recs"]
    r.view(torch.int32)[:14].fill_(3)           # the first record is written, the rest declared untouched
    A.check_untouched("recs", [(56, 168)])
    r.u8[100] = 0
    with pytest.raises(ArenaError) as ei:
        A.check_untouched("recs", [(56, 168)])
    assert "recs: byte 100 inside the region" in str(ei.value)
    A.check_untouched("recs", [(56, 100), (101, 168)])
    A.check()                                   # (the guards do not see it: that is what check_untouched is for)
    # against a snapshot instead of the pattern (an in-place call that must leave parts of its input alone)
    before = A.snapshot("recs")
    r.u8[7] = 9
    A.check_untouched("recs", [(8, 168)], expect=before)
    with pytest.raises(ArenaError) as ei:
        A.check_untouched("recs", [(0, 56)], expect=before)
    assert "recs: byte 7 " in str(ei.value)
    with pytest.raises(ArenaError):
        A.check_untouched("recs", [(0, 169)])


def test_write_into_a_snapshotted_input_is_caught():
    A = _arena()
    A["in"].fill_from(np.arange(5, dtype=np.uint64))
    A.snapshot_all(["in", "seqs"])
    A.assert_all_unchanged()
    A["in"].u8[33] ^= 1
    with pytest.raises(ArenaError) as ei:
        A.assert_unchanged("in")
    assert "in: input changed at byte 33" in str(ei.value)
    with pytest.raises(ArenaError):
        A.assert_all_unchanged()
    A.assert_unchanged("seqs")
    with pytest.raises(ArenaError):
        A.assert_unchanged("ws")                # never snapshotted


def test_other_garbage_in_the_guards():
    """an arena whose guards (and pre-filled outputs) hold another byte: the old pattern is a foreign byte there"""
    A = Arena(1 << 12, pattern=0xFF)
    r = A.carve("seqs", 48, 16).fill(0x41)
    assert bool((r.u8 == 0x41).all()) and int(A.buf[r.end]) == 0xFF and int(A.buf[0]) == 0xFF
    A.check()
    _poke(A, r.end, PATTERN)
    assert A.guard_faults() == [("seqs", "after", 0, PATTERN)]
