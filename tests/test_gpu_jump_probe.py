"""GPU parity of the jump table's probe as a quad fetch (k_runs.hip jump_probe_wave, rbg_jump.h jump_bucket): every lane of a wave enters
the probe, the four lanes of a quad fetch the bucket of each of them in turn, and the owner settles both slots from the sixteen words.  The
shapes are the smallest at which a cooperative fetch can go wrong: partial quads, a partial last wave, more than one workgroup, a second
and third round of the grid-stride loop, and quads that hold hits, absent keys, reads too short to probe and lanes without a read, every
kind in every lane position.  lo / hi / toehold bit for bit against the oracle's find_range_w_toehold and against the same replica loaded
without the table.  The kernel is the one the bench runs (rbg_find_range_w_toehold_dev: byte form, staged reads, 4-byte positions)."""
import numpy as np
import pytest

import orc
import rowbowt_amd as ra
from test_gpu_jump_table import ST_FTAB, ST_SYMBOLS, _dev_search, _load

pytestmark = pytest.mark.gpu
KS = (16, 60, 64)
NS = (1, 3, 5, 63, 64, 65, 513)


@pytest.fixture(scope="module")
def world(synth):
    """the oracle, the replica without the table and one replica per K with it (loaded once, shared, closed at the end)"""
    S = synth
    w = {"S": S, "o": orc.Oracle.from_runs(S.heads, S.lens, S.ssa, S.esa), "off": _load(S, 0)}
    for K in KS:
        w[K] = _load(S, K)
        assert w[K].jump_info().k == K and w[K].jump_info().keys > 0
    yield w
    for K in KS:
        w[K].close()
    w["off"].close()
    w["o"].close()


def _prep(seqs, off):
    """the batch and its three output arrays on the device"""
    import torch
    N = len(off) - 1
    dev = torch.device("cuda:0")
    d_seqs = torch.from_numpy(np.concatenate([seqs, np.zeros((-len(seqs)) % 16 + 16, np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    out = tuple(torch.full((max(N, 1),), -7, dtype=torch.int64, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    return N, d_seqs, d_off, out


def _launch(rb, prep, stream):
    """rbg_find_range_w_toehold_dev on `stream` (not synchronised): the tensors (lo, hi, k)"""
    N, d_seqs, d_off, out = prep
    assert ra.lib().rbg_find_range_w_toehold_dev(rb.h, d_seqs.data_ptr(), d_off.data_ptr(), N, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                 stream.cuda_stream) == 0
    return out


def _search(rb, seqs, off):
    import torch
    prep = _prep(seqs, off)
    out = _launch(rb, prep, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return out


def _host(out, N):
    return tuple(t.cpu().numpy().view(np.uint64)[:N] for t in out[:3])


def _check(w, K, reads, want=None):
    """the batch through the replica with the table and the one without: both equal the oracle, bit for bit"""
    seqs, off = ra.pack_reads(reads)
    N = len(reads)
    if want is None:
        want = w["o"].find_range_w_toehold_batch(seqs, off)
    got = _host(_search(w[K], seqs, off), N)
    plain = _host(_search(w["off"], seqs, off), N)
    for name, g, p, x in zip(("lo", "hi", "toehold"), got, plain, want):
        assert (g == x).all(), (K, N, name, np.flatnonzero(g != x)[:8])
        assert (p == x).all(), (K, N, name, "table off", np.flatnonzero(p != x)[:8])
    return want


def _sub(read, pos):
    return read[:pos] + bytes([next(c for c in b"ACGT" if c != read[pos])]) + read[pos + 1:]


def _kinds(S, K, rng):
    """makers of one read of each kind: too short to probe (K - 1), hits of K, K + 1 and K + 8 symbols, an absent key (a substitution inside
    the last K symbols), a hit that dies in the steps (a substitution before the last K symbols)"""
    text = S.text.tobytes()
    unit = S.L + S.pad

    def frag(m):
        s = int(rng.integers(S.H)) * unit + int(rng.integers(0, S.L - m + 1))
        return text[s:s + m]
    return [lambda: frag(K - 1), lambda: frag(K), lambda: frag(K + 1), lambda: frag(K + 8),
            lambda: _sub(frag(K + 8), 8 + int(rng.integers(K))), lambda: _sub(frag(K + 8), int(rng.integers(8)))]


def _mixed(S, K, N, shift, seed):
    """read i sits in quad q = i // 4 at position p = i % 4: every quad holds four different kinds, rotated by one lane from quad to quad
    (and by `shift`), the window of four kinds sliding over the six every four quads -- every kind meets every lane position"""
    rng = np.random.default_rng(seed)
    kinds = _kinds(S, K, rng)
    return [kinds[((i // 16) + ((i % 4 + i // 4 + shift) % 4)) % 6]() for i in range(N)]


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_probe_mixed_quads(world, K, N):
    """hits, absent keys, non-probing reads and (N not a multiple of four) lanes without a read in one quad, each kind in each of the four
    lane positions; N = 1 .. 513: partial quads, a partial last wave, two workgroups"""
    S = world["S"]
    for shift in range(4):
        reads = _mixed(S, K, N, shift, seed=1000 * K + 10 * N + shift)
        want = _check(world, K, reads)
        if N >= 63:
            lo, hi, _ = want
            assert (lo <= hi).any() and (lo > hi).any()


@pytest.mark.parametrize("K", KS)
def test_probe_counts_buckets_and_symbols(world, K):
    """the instrumented instantiation: every probing read reads at least one bucket, a read that does not probe none; every hit of the
    table consumes K symbols by the probe -- reads of exactly K symbols that occur are answered without a step"""
    S = world["S"]
    reads = S.sample_reads(130, K, seed=K, sub_rate=0.0) + S.sample_reads(70, K - 1, seed=K + 1, sub_rate=0.0) + [b""] * 3
    seqs, off = ra.pack_reads(reads)
    wlo, whi, wk = world["o"].find_range_w_toehold_batch(seqs, off)
    lo, hi, k, st = _dev_search(world[K], seqs, off, True)
    assert (lo == wlo).all() and (hi == whi).all() and (k == wk).all()
    assert 130 <= st[ST_FTAB] <= 3 * 130 + 70, st          # (a short read takes at most one ftab entry and no bucket)
    assert st[ST_SYMBOLS] >= 130 * K


@pytest.mark.parametrize("K", KS)
def test_probe_beside_a_wave_on_the_byte_walk(world, K):
    """three waves; one read of the middle wave holds an N, so that wave walks bytes (it never probes) beside two waves that probe"""
    S = world["S"]
    reads = _mixed(S, K, 192, 0, seed=77 + K)
    reads[70] = reads[70][:-3] + b"N" + reads[70][-2:]
    _check(world, K, reads)


@pytest.mark.parametrize("K", KS)
def test_probe_wave_of_misses_and_wrapped_toeholds(world, K):
    """every read of the second wave has an absent key (a substitution inside its last K symbols); the first wave holds the text's prefixes,
    whose toeholds wrap below zero and travel as 0xFFFFFFFF in the table"""
    S = world["S"]
    rng = np.random.default_rng(K)
    kinds = _kinds(S, K, rng)
    text = S.text.tobytes()
    first = [text[:m] for m in (K, K + 1, K + 8)] + [kinds[i % 4]() for i in range(61)]
    misses = [kinds[4]() for _ in range(64)]
    lo, hi, k = _check(world, K, first + misses)
    assert (lo[:3] <= hi[:3]).all()
    assert (lo[64:] > hi[64:]).sum() >= 60                                    # (a substituted K-mer may occur by chance)


def test_probe_three_rounds_of_the_grid_stride_loop(world):
    """a batch of more than two strides of the grid (most reads empty, so the oracle stays quick): wave 0 meets 64 absent keys in each of its
    three rounds -- 192 misses in one wave's stride -- and its neighbours mixed quads in the second and third round"""
    import torch
    S, K = world["S"], 16
    stride = (torch.cuda.get_device_properties(0).multi_processor_count * 32 // 2) * 512      # (launch_find_range_runs_impl: 512-thread workgroups)
    N = 2 * stride + 321
    rng = np.random.default_rng(5)
    kinds = _kinds(S, K, rng)
    lens = np.zeros(N, np.int64)
    parts = []
    for r in range(3):
        batch = [kinds[4]() for _ in range(64)] + _mixed(S, K, 257, r, seed=900 + r)
        lens[r * stride:r * stride + len(batch)] = [len(b) for b in batch]
        parts += batch
    seqs = np.frombuffer(b"".join(parts), np.uint8).copy()
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    want = world["o"].find_range_w_toehold_batch(seqs, off, nthreads=4)
    got = _host(_search(world[K], seqs, off), N)
    plain = _host(_search(world["off"], seqs, off), N)
    for g, p, x in zip(got, plain, want):
        assert (g == x).all() and (p == x).all()
    for r in range(3):
        assert (want[0][r * stride:r * stride + 64] > want[1][r * stride:r * stride + 64]).sum() >= 55
        assert (want[0][r * stride + 64:r * stride + 321] <= want[1][r * stride + 64:r * stride + 321]).any()


def test_probe_two_streams_one_handle(world):
    """two batches on two streams through one replica at the same time: the probe keeps no state outside the wave, so each batch gets what it
    gets alone"""
    import torch
    S, K = world["S"], 60
    batches = [_mixed(S, K, 4099, s, seed=40 + s) for s in (0, 1)]
    packed = [ra.pack_reads(b) for b in batches]
    alone = [_host(_search(world[K], seqs, off), len(off) - 1) for seqs, off in packed]
    preps = [_prep(seqs, off) for seqs, off in packed]
    outs = [_launch(world[K], prep, torch.cuda.Stream()) for prep in preps]
    torch.cuda.synchronize()
    for (seqs, off), a, out in zip(packed, alone, outs):
        both = _host(out, len(off) - 1)
        want = world["o"].find_range_w_toehold_batch(seqs, off)
        for g, x, y in zip(both, a, want):
            assert (g == x).all() and (g == y).all()
