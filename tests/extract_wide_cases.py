"""Test infrastructure: the two inputs of tests/test_gpu_extract_wide.py and every value its legs compare against, made without a device and without the
library's extract (tests/test_extract_wide_expected.py runs all of it where no GPU exists).

  W  wide(): a true BWT with n > 2^32 whose text is never written out -- rowbowt_amd.tools.pangenome_bwt: 2 000 haplotypes of 2.2 M bases, the run list from
     build_runs, text[pos] from TextView.  Its only byte that is no base is the terminator, so the ISA samples are the runs' last rows and the structure of
     rbg_isa.hpp follows in numpy: tpos = sort(esa), the row of sample j = run_start[i + 1] - 1 of its run, dir[b] by searchsorted, the sample before p by
     searchsorted(tpos, p, 'right') - 1.  Rows come from the CPU oracle over the same run list (LF of a sample's row; ranges and locations of reads).
  D  docs(): 251 documents with 4-byte positions through isa_model.Text (naive suffix array): near copies of one 240-base sequence joined by '#', with
     documents that start with N, that end with N ("N#"), that hold a run of 1 to 39 N, one empty document ("##"), N as the text's first byte.

Each leg's values come from a function of its own that also asserts, from the expected values alone, that the leg reaches the edge it is for."""
import functools
import itertools
import types

import numpy as np
import torch

import isa_model as IM
import orc
from rowbowt_amd.tools import pangenome_bwt as PB

TWO31, TWO32 = 1 << 31, 1 << 32
STEP_CAP = 2_000_000_000                  # FL steps one device call of a leg may take (0.12 s at the 1.66e10 steps/s of DESIGN 6j): a condition, not a measurement
LENS = IM.LENS + (150, 1000)              # the interval lengths of W's items
OUT_LENS = (1, 15, 16, 17, 33, 70)        # ... and of the items whose out_off crosses 2^32
BIG_OUT = TWO32 + (1 << 20)               # bytes of that leg's output buffer
ACGT = np.frombuffer(b"ACGT", np.uint8)
FILL = 0xA5
READ_LEN = 100


# ---- W ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide():
    pg = PB.make_pangenome(L=2_200_000, H=2000, site_rate=0.001, seed=5, device="cpu")
    runs = PB.build_runs(pg)
    W = types.SimpleNamespace(pg=pg, text=PB.TextView(pg), n=int(runs["n"]), r=int(runs["r"]), heads=runs["heads"], lens=runs["lens"], ssa=runs["ssa"],
                              esa=runs["esa"], L=pg["L"], H=pg["H"], unit=pg["unit"])
    n, r = W.n, W.r
    lens, esa = W.lens.astype(np.int64), W.esa.astype(np.int64) % n
    start = np.zeros(r + 1, np.int64)
    start[1:] = np.cumsum(lens)
    assert int(start[r]) == n
    W.second_kind = int((lens[~np.isin(W.heads, ACGT)] - 1).sum())
    assert W.second_kind == 0, "a run of a byte that is no base holds several rows: the samples are no longer the runs' last rows alone"
    W.run = np.argsort(esa, kind="stable")                    # the run of sample j
    W.tpos, W.row = esa[W.run], (start[1:] - 1)[W.run]
    W.samples = S = r
    W.shift = 0
    while (S << (W.shift + 1)) <= n:
        W.shift += 1
    W.dir_entries = (n >> W.shift) + 2
    W.dir = np.searchsorted(W.tpos, np.arange(W.dir_entries, dtype=np.int64) << W.shift, "right") - 1
    W.gap = np.diff(np.append(W.tpos, n))
    W.max_gap = int(W.gap.max())
    W.bucket = np.bincount(W.tpos >> W.shift, minlength=(n >> W.shift) + 1)       # samples per bucket of 2^shift positions
    W.bytes = S * 2 * 8 + W.dir_entries * 8
    return W


def wide_shapes(W):
    """the shapes the legs rely on, as conditions: a change of the generator cannot quietly take the case away"""
    assert W.n > TWO32 and int(W.tpos[0]) == 0 and (W.gap > 0).all()
    assert int((W.tpos < TWO32).sum()) >= 1000 and int((W.tpos >= TWO32).sum()) >= 1000
    assert int(W.bucket.max()) >= 256, "no directory bucket holds 256 samples: the long bisection is missing"
    assert int((W.bucket == 0).sum()) * 2 >= len(W.bucket), "fewer than half of the buckets are empty"
    assert W.max_gap >= 20_000
    assert ((W.tpos < TWO32) & (W.tpos + W.gap > TWO32)).any(), "no gap starts below 2^32 and ends above it"
    assert (W.dir >= 0).all() and int(W.dir[-1]) == W.samples - 1 and int(W.row.max()) >= TWO32 and W.shift >= 8


def before(W, p):
    """the index of the sample before each position"""
    return np.searchsorted(W.tpos, p, "right") - 1


def walk_in(W, p):
    """FL steps from the sample before each position"""
    p = np.asarray(p, np.int64)
    return p - W.tpos[before(W, p)]


def bytes_at(W, idx):
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    return W.text.at(torch.from_numpy(idx)).numpy()


def wide_bytes(W, pos, length):
    """(the bytes of every interval, one after the other: text[p:p + len] up to the terminator, then zeros -- isa_model.expected on a text whose only byte
    that is no base is the terminator --, got)"""
    pos, length = np.asarray(pos, np.int64), np.asarray(length, np.int64)
    item = np.repeat(np.arange(len(pos)), length)
    idx = pos[item] + (np.arange(int(length.sum())) - np.repeat(np.cumsum(length) - length, length))
    live = idx < W.n - 1
    flat = np.zeros(len(idx), np.uint8)
    flat[live] = bytes_at(W, idx[live])
    assert np.isin(flat[live], ACGT).all()
    return flat, np.clip(W.n - 1 - pos, 0, length)


def layout(length, at=3, k0=0):
    """out_off of items laid out with gaps of 1 .. 17 bytes -> (off, the first byte behind the last item)"""
    off, end = np.zeros(len(length), np.int64), at
    for k, L in enumerate(np.asarray(length).tolist()):
        off[k], end = at, at + L
        at = end + 1 + ((k0 + k + 1) % 17)
    return off, end


def scatter(want, base, off, length, flat):
    """the items' bytes into want[off - base ...]"""
    off, length = np.asarray(off, np.int64), np.asarray(length, np.int64)
    dst = np.repeat(off - base, length) + (np.arange(int(length.sum())) - np.repeat(np.cumsum(length) - length, length))
    want[dst] = flat


@functools.lru_cache(maxsize=None)
def oracle():
    W = wide()
    return orc.Oracle.from_runs(W.heads, W.lens, W.ssa, W.esa)


def wide_info(W):
    """leg a"""
    assert W.bytes == W.samples * 2 * 8 + W.dir_entries * 8 and W.dir_entries == (W.n >> W.shift) + 2
    return dict(prepared=True, bytes=W.bytes, samples=W.samples, shift=W.shift, dir_entries=W.dir_entries, second_kind=W.second_kind, max_gap=W.max_gap)


def _largest_gap(W):
    jg = int(np.argmax(W.gap))
    return int(W.tpos[jg]), int(W.tpos[jg]) + W.max_gap        # [its sample, the next sample or n)


@functools.lru_cache(maxsize=None)
def wide_samples():
    """leg b: every sample position with its row (no walk), and the position before a sample -- the longest walk its gap allows -- for the 2 000 samples nearest
    2^32, the fullest bucket's and the one that ends the largest gap; its row is LF of the sample's row, from the oracle"""
    W, o = wide(), oracle()
    near = np.argsort(np.abs(W.tpos - TWO32), kind="stable")[:2000]
    b = int(np.argmax(W.bucket))
    full = np.arange(int(np.searchsorted(W.tpos, b << W.shift)), int(np.searchsorted(W.tpos, (b + 1) << W.shift)))
    assert len(full) == int(W.bucket.max()) and int(W.dir[b + 1]) - int(W.dir[b]) >= len(full) - 1
    g0, g1 = _largest_gap(W)
    assert g1 < W.n, "the largest gap is the text's last: no sample ends it"
    J = np.unique(np.concatenate([near, full, [int(before(W, g1))]]))
    J = J[W.tpos[J] > 0]
    p = W.tpos[J] - 1
    c = W.heads[W.run[J]]
    assert np.isin(c, ACGT).all()
    lo, hi = o.LF_batch(W.row[J].astype(np.uint64), W.row[J].astype(np.uint64), c)
    assert (lo == hi).all()
    want = lo.astype(np.int64)
    steps = walk_in(W, p)
    assert (steps == W.gap[J - 1] - 1).all() and int(steps.max()) == W.max_gap - 1 and int(steps.sum()) < STEP_CAP
    assert (p < TWO32).sum() >= 100 and (p >= TWO32).sum() >= 100 and (want >= TWO32).any() and (want < TWO32).any()
    # where the position before a sample is a sample itself, the oracle's LF must give that sample's row: the two sources agree
    adj = np.flatnonzero(steps == 0)
    assert len(adj) >= 100 and (want[adj] == W.row[J[adj] - 1]).all()
    return types.SimpleNamespace(pos=W.tpos, row=W.row, before_pos=p, before_row=want, steps=int(steps.sum()), longest=int(steps.max()))


def _carried_sites(W, count, seed):
    """(haplotype, offset) of variant sites the haplotype carries, haplotypes on both sides of 2^32"""
    rng = np.random.default_rng(seed)
    G, sites = W.pg["G"].numpy(), W.pg["sites"].numpy()
    out = []
    hs = np.stack([rng.integers(1, W.H, count), rng.integers(TWO32 // W.unit + 1, W.H, count)], axis=1).ravel()[:count]
    for h in hs.tolist():
        js = np.flatnonzero(G[:, h])
        out.append((h, int(sites[js[int(rng.integers(0, len(js)))]])))
    assert any(h * W.unit > TWO32 for h, _ in out) and any(h * W.unit + W.unit < TWO32 for h, _ in out)
    return out


@functools.lru_cache(maxsize=None)
def wide_locate():
    """leg c: reads of 100 bases read off the text; the oracle's range [lo, hi] and locations SA[hi], SA[hi - 1], ... (include/rbg.h) give isa(locs[j]) ==
    hi - j.  The reads are kept in their round-robin order as long as the walk-ins of their locations stay below STEP_CAP"""
    W, o = wide(), oracle()
    rng = np.random.default_rng(20261)
    L, H, unit, n = W.L, W.H, W.unit, W.n
    g0, g1 = _largest_gap(W)
    span = L - READ_LEN
    kinds = {
        "below 2^32": rng.integers(0, TWO32 - READ_LEN, 57),
        "above 2^32": rng.integers(TWO32, n - 1 - READ_LEN, 60),
        "around 2^32": TWO32 + np.array([-99, -64, -50, -37, -1, 0, 3, 700]),
        "largest gap": g1 - READ_LEN - 7 * np.arange(10),
        "last haplotype": np.append((H - 1) * unit + rng.integers(0, span, 39), n - 1 - READ_LEN),
        "haplotype 0": np.append(rng.integers(0, span, 39), 0),
        "carried site": np.array([h * unit + min(max(s - int(rng.integers(0, READ_LEN)), 0), span) for h, s in _carried_sites(W, 85, 20262)]),
    }
    assert g0 <= int(kinds["largest gap"].min()) and sum(len(v) for v in kinds.values()) == 300
    names = list(kinds)
    order = [kv for tup in itertools.zip_longest(*[[(i, int(x)) for x in kinds[k]] for i, k in enumerate(names)]) for kv in tup if kv is not None]
    kind = np.array([i for i, _ in order])
    starts = np.array([v for _, v in order], np.int64)
    reads = bytes_at(W, starts[:, None] + np.arange(READ_LEN)[None, :])
    assert np.isin(reads, ACGT).all()
    seqs, off = orc.pack_reads([bytes(q) for q in reads])
    lo, hi, k = o.find_range_w_toehold_batch(seqs, off)
    assert (hi >= lo).all() and int((hi - lo).max()) < H + 50, "a read taken from the text does not occur, or occurs more often than there are haplotypes"
    loc_off, locs = o.locs_at_batch(lo, hi, k, orc.MAXU)
    loc_off, locs = loc_off.astype(np.int64), locs.astype(np.int64)
    read = np.repeat(np.arange(len(starts)), np.diff(loc_off))
    rows = hi.astype(np.int64)[read] - (np.arange(len(locs)) - loc_off[read])
    assert int(locs.max()) < n
    for i, s in enumerate(starts.tolist()):                 # text and oracle agree: every read is found where it was read
        assert s in locs[loc_off[i]:loc_off[i + 1]]
    steps = walk_in(W, locs)
    per_read = np.add.reduceat(steps, loc_off[:-1])
    keep = int(np.searchsorted(np.cumsum(per_read), STEP_CAP, "left"))
    m = int(loc_off[keep])
    pos, rows, steps, kind = locs[:m], rows[:m], steps[:m], kind[:keep]
    assert int(steps.sum()) < STEP_CAP and m >= 100_000 and keep >= 50
    assert set(kind.tolist()) == set(range(len(names))), "the step cap leaves no read of some kind"
    assert (pos < TWO32).sum() >= 1000 and (pos >= TWO32).sum() >= 1000 and (rows >= TWO32).any() and (rows < TWO32).any()
    assert int(steps.max()) >= 20_000 and ((pos >= g0) & (pos < g1)).any()
    assert ((pos >= TWO32) & (pos - steps < TWO32)).any(), "no walk starts at a sample below 2^32 and ends above it"
    return types.SimpleNamespace(pos=pos, row=rows, reads=keep, steps=int(steps.sum()), longest=int(steps.max()))


@functools.lru_cache(maxsize=None)
def wide_extract():
    """leg d: (pos, len, out_off) over a FILL-filled buffer, the expected buffer and got"""
    W = wide()
    rng = np.random.default_rng(20263)
    n, L, H, unit = W.n, W.L, W.H, W.unit
    g0, g1 = _largest_gap(W)
    near = np.sort(np.argsort(np.abs(W.tpos - TWO32), kind="stable")[:500])
    b = int(np.argmax(W.bucket))
    full = np.arange(int(np.searchsorted(W.tpos, b << W.shift)), int(np.searchsorted(W.tpos, (b + 1) << W.shift)))
    around = np.concatenate([W.tpos[j][:, None] + np.array([-1, 0, 1])[None, :] for j in (near, full)]).ravel()
    sites = np.array([h * unit + s + d for h, s in _carried_sites(W, 200, 20264) for d in (-1, 0, 1)])
    d = np.arange(-40, 41)
    pos = np.concatenate([
        [0, 1, n - 2, n - 1], TWO31 + d, TWO32 + d, [g0, g1 - 1], around[(around >= 0) & (around < n)],
        np.arange((H - 2) * unit + L - 3, (H - 1) * unit + 3),            # the pad between the last two haplotypes
        np.arange(n - 200, n), sites, rng.integers(0, TWO32, 10_000), rng.integers(TWO32, n, 10_000)]).astype(np.int64)
    assert int(pos.min()) == 0 and int(pos.max()) == n - 1
    length = np.array(LENS, np.int64)[np.arange(len(pos)) % len(LENS)]
    off, end = layout(length)
    total = end + 5
    flat, got = wide_bytes(W, pos, length)
    want = np.full(total, FILL, np.uint8)
    scatter(want, 0, off, length, flat)
    steps = int(walk_in(W, pos).sum()) + int(length.sum())
    assert steps < STEP_CAP
    assert set((off % 16).tolist()) == set(range(16)) and set((off[length > 20] % 16).tolist()) == set(range(16))
    assert set((off[1:] - off[:-1] - length[:-1]).tolist()) == set(range(1, 18))
    assert (pos >= TWO32).sum() >= 10_000 and ((pos < TWO32) & (pos + length > TWO32)).any() and ((pos < TWO31) & (pos + length > TWO31)).any()
    assert ((got < length) & (got > 0)).any() and ((got == 0) & (length > 0)).any() and (got[length == 1000] == 1000).any()
    assert int(walk_in(W, pos).max()) == W.max_gap - 1
    for L_ in LENS:                                                        # every length at a position above 2^32
        assert ((length == L_) & (pos >= TWO32)).any()
    return types.SimpleNamespace(pos=pos, length=length, off=off, want=want, got=got, steps=steps, sub=slice(0, 1024))


@functools.lru_cache(maxsize=None)
def wide_out_off():
    """leg e: 400 items in a buffer of 2^32 + 2^20 bytes: from offset 3, from 2^31 - 35, through 2^32 - 64 .. 2^32 + 64 with a start at every residue mod 4
    and one item across 2^32 itself, the last one up to the buffer's last byte -> the items and the expected bytes of the windows that hold them"""
    W = wide()
    rng = np.random.default_rng(20265)
    pos = np.concatenate([rng.integers(0, TWO32, 200), rng.integers(TWO32, W.n - 100, 200)])
    rng.shuffle(pos)
    length = np.array(OUT_LENS, np.int64)[np.arange(400) % len(OUT_LENS)]
    length[100] = 70                                                       # from 2^31 - 35 across 2^31
    off = np.zeros(400, np.int64)
    off[0:100], _ = layout(length[0:100], 3)
    off[100:200], _ = layout(length[100:200], TWO31 - 35, 100)
    # through 2^32: each start the first offset behind the item before it with the residue of its turn
    length[200:206] = (15, 17, 1, 70, 16, 33)
    at = TWO32 - 64
    for k in range(200, 300):
        while at % 4 != k % 4:
            at += 1
        off[k] = at
        at += int(length[k]) + 1
    off[300:400], end = layout(length[300:400], BIG_OUT - 64 * 1024, 300)
    off[399] = BIG_OUT - int(length[399])
    assert off[398] + length[398] < off[399] and (off[1:] >= off[:-1] + length[:-1] + 1).all()
    flat, got = wide_bytes(W, pos, length)
    assert (got == length).all()
    windows = []
    for a, z, sl in ((0, 1 << 16, slice(0, 100)), (TWO31 - (1 << 15), TWO31 + (1 << 15), slice(100, 200)), (TWO32 - (1 << 15), TWO32 + (1 << 15), slice(200, 300)),
                     (BIG_OUT - (1 << 17), BIG_OUT, slice(300, 400))):
        assert a <= int(off[sl].min()) - 3 and int((off[sl] + length[sl]).max()) <= z
        want = np.full(z - a, FILL, np.uint8)
        f0 = int(length[:sl.start].sum())
        scatter(want, a, off[sl], length[sl], flat[f0:f0 + int(length[sl].sum())])
        windows.append((a, z, want))
    ends = off + length
    inside = (ends > TWO32 - 64) & (off < TWO32 + 64)
    assert inside.sum() >= 4 and set((off[inside] % 4).tolist()) == {0, 1, 2, 3}
    assert ((off < TWO32) & (ends > TWO32 + 4) & (length >= 33)).sum() == 1 and ((off < TWO31) & (ends > TWO31)).any()
    assert (off >= TWO32).sum() >= 100 and int(off[0]) == 3 and int(off[100]) == TWO31 - 35 and int(ends[399]) == BIG_OUT
    assert (pos[off >= TWO32] >= TWO32).any() and (pos[off >= TWO32] < TWO32).any() and set(length.tolist()) == set(OUT_LENS)
    assert int(walk_in(W, pos).sum()) + int(length.sum()) < STEP_CAP
    return types.SimpleNamespace(pos=pos, length=length, off=off, got=got, windows=windows, nbytes=int(length.sum()))


@functools.lru_cache(maxsize=None)
def wide_host():
    """leg f: the intervals of the host call with their bytes and got"""
    W = wide()
    h = TWO32 // W.unit + 8
    assert h * W.unit > TWO32 and h < W.H - 1
    iv = {"across 2^32": (TWO32 - 5000, 10_000), "haplotype": (h * W.unit, W.unit), "the end": (W.n - 300, 1000)}
    out = {}
    for name, (p, l) in iv.items():
        flat, got = wide_bytes(W, [p], [l])
        out[name] = (p, l, flat.tobytes(), int(got[0]))
    assert out["the end"][3] == 299 and out["the end"][2][299:] == bytes(701) and out["haplotype"][3] == W.unit and out["across 2^32"][3] == 10_000
    pieces = sum(-(-l // 128) for _, l, _, _ in out.values()) + 10_000 + -(-10_000 // 7)
    assert pieces * W.max_gap < 40 * STEP_CAP      # (a bound, loose: the pieces' mean walk-in is a fraction of the largest gap)
    return out


# ---- D ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def docs():
    rng = np.random.default_rng(250)
    base = rng.choice(ACGT, 240)
    out = []
    for d in range(250):
        s = base.copy()
        for at in rng.choice(240, 3, replace=False).tolist():
            s[at] = ACGT[(int(np.flatnonzero(ACGT == s[at])[0]) + 1 + int(rng.integers(0, 3))) % 4]
        if d % 5 == 0:
            k = 1 + ((d // 5) * 7) % 39
            at = 20 + int(rng.integers(0, 160))
            s[at:at + k] = ord("N")
        if d % 7 == 0:
            s[0] = ord("N")
        if d % 11 == 0:
            s[-1] = ord("N")
        out.append(s.tobytes())
    out.insert(100, b"")                                                   # the empty document: "##"
    text = b"#".join(out) + b"\x01"
    starts = np.cumsum([0] + [len(s) + 1 for s in out[:-1]]).tolist()
    T = IM.Text(text, [f"d{j}" for j in range(len(out))], starts)
    T.docs = out
    assert T.n == 250 * 240 + 250 + 1 < TWO31 and text[0] == ord("N") and b"##" in text and b"N#" in text and b"N" * 39 in text
    return T


@functools.lru_cache(maxsize=None)
def docs_model():
    M = docs().model()
    assert M.second_kind >= 1000 and M.longest_other_run >= 100
    return M


@functools.lru_cache(maxsize=None)
def docs_extract():
    """leg g: every position with every length of isa_model.LENS -> the items, the expected buffer and got; every kind of stop asserted present"""
    T = docs()
    t = T.text
    stop = np.flatnonzero(~np.isin(t, ACGT))
    p = np.arange(T.n)
    bases = stop[np.searchsorted(stop, p)] - p                            # bases from p up to the first byte that is none
    pos = np.repeat(p, len(IM.LENS))
    length = np.tile(np.array(IM.LENS, np.int64), T.n)
    got = np.minimum(length, bases[pos])
    off, end = layout(length)
    want = np.full(end + 5, FILL, np.uint8)
    scatter(want, 0, off, length, np.zeros(int(length.sum()), np.uint8))
    scatter(want, 0, off, got, t[np.repeat(pos, got) + (np.arange(int(got.sum())) - np.repeat(np.cumsum(got) - got, got))])
    s = pos[got < length] + got[got < length]                             # where a walk stopped
    nxt = np.append(t[1:], 0)
    kinds = {"#": (t[s] == ord("#")), "inside a run of N": (t[s] == ord("N")) & (nxt[s] == ord("N")), "N#": (t[s] == ord("N")) & (nxt[s] == ord("#")),
             "##": (t[s] == ord("#")) & (nxt[s] == ord("#")), "the leading N": s == 0, "the terminator": t[s] == 1}
    for what, m in kinds.items():
        assert m.any(), f"no walk ends at {what}"
    assert set((off % 16).tolist()) == set(range(16))
    return types.SimpleNamespace(pos=pos, length=length, off=off, want=want, got=got)


def docs_documents():
    """every document by its bounds (its separator or the terminator included): the document's text up to its first N"""
    T = docs()
    ends = list(T.doc_starts[1:]) + [T.n]
    pos, length = np.array(T.doc_starts, np.uint64), np.array([e - s for s, e in zip(T.doc_starts, ends)], np.uint64)
    want = [d.split(b"N")[0] for d in T.docs]
    assert sum(len(w) < len(d) for w, d in zip(want, T.docs)) >= 50 and want[0] == b"" and want[100] == b"" and T.docs[100] == b""
    return pos, length, want
