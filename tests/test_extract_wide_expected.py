"""The CPU half of tests/test_gpu_extract_wide.py where no GPU exists (tests/extract_wide_cases.py): the two inputs are built and held to the shapes the
device legs are about, every leg's value function runs -- each asserts that its values reach the edge it is for --, W's numpy directory and lookup are held
to their definitions, and D's values to isa_model: its ISA to the naive one at every position, isa_model.expected to the model's extract at every
position and length.  No device is touched."""
import numpy as np

import extract_wide_cases as C
import isa_model as IM


def test_wide_input_has_the_shapes_the_legs_are_about():
    W = C.wide()
    C.wide_shapes(W)
    assert C.wide_info(W)["bytes"] == W.samples * 16 + W.dir_entries * 8
    # the directory and the lookup in numpy, against their definitions at chosen buckets and positions
    rng = np.random.default_rng(1)
    full = int(np.argmax(W.bucket))
    for b in [0, 1, full, full + 1, W.dir_entries - 2, W.dir_entries - 1, C.TWO32 >> W.shift, (C.TWO32 >> W.shift) - 1] + rng.integers(0, W.dir_entries, 200).tolist():
        j = int(W.dir[b])
        assert int(W.tpos[j]) <= (b << W.shift) and (j + 1 == W.samples or int(W.tpos[j + 1]) > (b << W.shift))
    assert int(W.dir[full + 1]) - int(W.dir[full]) >= 255                                    # a bisection over hundreds of samples
    p = np.concatenate([[0, W.n - 1, C.TWO32 - 1, C.TWO32], rng.integers(0, W.n, 1000)])
    j = C.before(W, p)
    assert (W.tpos[j] <= p).all() and (np.append(W.tpos, W.n)[j + 1] > p).all()
    assert ((W.dir[p >> W.shift] <= j) & (j <= W.dir[(p >> W.shift) + 1])).all()              # the answer lies in the bucket's pair
    assert (C.walk_in(W, p) < W.max_gap).all() and int(C.walk_in(W, W.tpos).max()) == 0
    # the text view: the terminator last, pads of A, the base sequence in haplotype 0
    assert C.bytes_at(W, [W.n - 1, W.n - 2, W.L, W.unit - 1]).tolist() == [1, 65, 65, 65]
    assert (C.bytes_at(W, np.arange(1000)) == np.frombuffer(b"ACGT", np.uint8)[W.pg["base"][:1000].numpy()]).all()


def test_wide_legs_reach_their_edges():
    W = C.wide()
    b = C.wide_samples()
    assert len(b.pos) == W.r and b.longest == W.max_gap - 1
    c = C.wide_locate()
    assert 100_000 <= len(c.pos) <= 1_000_000 and c.steps < C.STEP_CAP
    d = C.wide_extract()
    assert len(d.pos) > 20_000 and len(d.want) == int(d.off[-1] + d.length[-1]) + 5 and d.steps < C.STEP_CAP
    assert int((d.want != C.FILL).sum()) == int(d.length.sum())                             # every expected byte is a base or zero
    e = C.wide_out_off()
    assert len(e.pos) == 400 and sum(int((w != C.FILL).sum()) for _, _, w in e.windows) == e.nbytes
    f = C.wide_host()
    assert set(f) == {"across 2^32", "haplotype", "the end"}


def test_docs_input_against_the_model():
    T, M = C.docs(), C.docs_model()
    assert M.samples == len(T.heads) + M.second_kind and T.n == M.n
    rows = [M.isa(p) for p in range(T.n)]
    assert rows == T.isa.tolist()                                                            # (the issue asks for every 7th position at least: all of them)
    x = C.docs_extract()
    at = 0
    for p in range(T.n):
        for L in IM.LENS:
            want = IM.expected(T.tb, p, L)
            assert M.extract_from(rows[p], L) == want
            o = int(x.off[at])
            assert (int(x.pos[at]), int(x.length[at]), int(x.got[at])) == (p, L, want[1]) and x.want[o:o + L].tobytes() == want[0]
            at += 1
    assert at == len(x.pos) and int((x.want != C.FILL).sum()) == int(x.length.sum())
    pos, length, want = C.docs_documents()
    assert len(pos) == 251 and [IM.expected(T.tb, int(p), int(l))[0][:len(w)] for p, l, w in zip(pos, length, want)] == want
    assert all(IM.expected(T.tb, int(p), int(l))[1] == len(w) for p, l, w in zip(pos, length, want))
