"""Inputs and the counter model for the suffix-array build past one grid pass (rowbowt_amd/csrc/sa_build.hip; tests/test_gpu_sa_build_scale.py, its CPU
half tests/test_sa_scale_expected.py).  Everything here is numpy on the CPU from fixed seeds; no device, no torch.

Every kernel of sa_build.hip strides a grid that sa_grid caps at 8 192 workgroups of 256 lanes: CAP = 2 097 152 lanes.  A text of n <= CAP symbols gives
every lane one element; the texts of this module put n at CAP - 1, CAP, CAP + 1 and 2 CAP + 1 (a third pass that holds one element), at rocPRIM's
merge-sort limit 2^20 and one above it, and past CAP with nearly every suffix still tied after the first key (near_copies_at_scale) or with every suffix
tied up to the last round (long_run).

The counter model.  The build sorts by 8 symbols in round 0 and doubles the depth every round; a suffix leaves the work list once no other suffix shares
its first 8 * 2^k symbols, that is once both common prefixes with its suffix-array neighbours are shorter.  With lcp[j] the common prefix of rows j - 1
and j (lcp[0] = lcp[n] = 0):
    m_k              = #{ rows j : max(lcp[j], lcp[j + 1]) >= 8 * 2^k }
    tied_after_first = m_0
    rounds           = 1 + the first k with m_k = 0
    sorted           = n + sum of m_k
(counter_model).  lcp_array is Kasai's array without Kasai's loop over Python integers: PLCP[i] = PLCP[i - 1] - 1 wherever the BWT byte of suffix i's
row equals that of the row before (Karkkainen, Manzini & Puglisi 2009, "Permuted longest-common-prefix array", lemma 1), so only the irreducible
positions -- one per BWT run -- are compared symbol by symbol, eight bytes at a step over packed big-endian keys.  doubling_simulation is the second,
plain implementation the model is held to: group-head prefix doubling over numpy arrays (rank = the first row of the group, singletons dropped), which
counts what it sorts."""
import functools

import numpy as np

CAP = 8192 * 256          # kSaGridCap workgroups of kSaThreads lanes (sa_build.hip)
MERGE_LIMIT = 1 << 20     # rocPRIM radix_sort: merge sort up to here, onesweep above (64-bit keys)
BOUNDARY_NS = (MERGE_LIMIT, MERGE_LIMIT + 1, CAP - 1, CAP, CAP + 1, 2 * CAP + 1)
ACGT = np.frombuffer(b"ACGT", np.uint8)
COPY_LEN, COPIES, SNVS = 100_000, 30, 100
LONG_RUN_AS = CAP + 300


def _t(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


@functools.lru_cache(maxsize=None)
def boundary_text(n):
    """random ACGT of length n - 1 and the terminator"""
    return np.append(np.random.default_rng(n).choice(ACGT, n - 1), 1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def near_copies_at_scale():
    """30 copies of one random 100 000-base sequence joined by '#': every fourth copy (0, 4, 8, ...) carries 100 SNVs, the others are the sequence itself
    -- tests/test_gpu_sa_build.py::near_copies at n = 3 000 030.  Copies 1-3 and 5-7 are verbatim, so two suffixes share 3 * 100 001 - 1 symbols"""
    rng = np.random.default_rng(30)
    base = rng.choice(ACGT, COPY_LEN)
    out = []
    for d in range(COPIES):
        s = base.copy()
        if d % 4 == 0:
            at = rng.choice(COPY_LEN, SNVS, replace=False)
            code = np.searchsorted(ACGT, s[at])
            s[at] = ACGT[(code + 1 + rng.integers(0, 3, SNVS)) % 4]
        out.append(s.tobytes())
    return _t(b"#".join(out) + b"\x01")


def long_run(k=LONG_RUN_AS):
    return _t(b"A" * k + b"\x01")


def long_run_sa(n):
    """the suffix array of A * (n - 1) + terminator in closed form: the terminator first, then the A suffixes from the shortest to the longest"""
    return np.arange(n - 1, -1, -1, dtype=np.int64)


def scale_texts():
    """name -> a function that makes the text (made on demand: 20 MB in all)"""
    T = {f"boundary n={n}": functools.partial(boundary_text, n) for n in BOUNDARY_NS}
    T["near copies at scale"] = near_copies_at_scale
    T["long run"] = long_run
    return T


def runs_from_sa(text, sa):
    """(heads u8[R], lens u64[R], ssa u64[R], esa u64[R]) of BWT[i] = text[(sa[i] - 1) mod n], byte 0 read as 1: the run builders' arrays"""
    text, sa = np.asarray(text, np.uint8), np.asarray(sa, np.int64)
    n = len(text)
    bwt = text[(sa - 1) % n]
    bwt = np.where(bwt == 0, 1, bwt).astype(np.uint8)
    starts = np.flatnonzero(np.append(True, bwt[1:] != bwt[:-1]))
    ends = np.append(starts[1:] - 1, n - 1)
    return bwt[starts], (ends - starts + 1).astype(np.uint64), sa[starts].astype(np.uint64), sa[ends].astype(np.uint64)


def pack_keys8(text):
    """K[i] = text[i .. i + 8) as one big-endian uint64, zeros behind the text: the build's first key"""
    text = np.asarray(text, np.uint8)
    n = len(text)
    pad = np.zeros(n + 8, np.uint64)
    pad[:n] = text
    K = np.zeros(n, np.uint64)
    for d in range(8):
        K = (K << np.uint64(8)) | pad[d:d + n]
    return K


def shared_first_keys(text):
    """the suffixes whose zero-padded 8-byte key is also another suffix's"""
    _, counts = np.unique(pack_keys8(text), return_counts=True)
    return int(counts[counts > 1].sum())


def _extend(text, a, b, length):
    """the common prefix of the suffixes at a and b, of which `length` symbols are known to agree: slices of growing size"""
    n, step = len(text), 256
    while True:
        m = min(step, n - max(a, b) - length)
        assert m > 0, (a, b, length)                   # (two suffixes differ before the shorter one ends)
        d = np.flatnonzero(text[a + length:a + length + m] != text[b + length:b + length + m])
        if d.size:
            return length + int(d[0])
        length, step = length + m, step * 4


def lcp_array(text, sa):
    """lcp[0 .. n]: lcp[j] = the common prefix of the suffixes at rows j - 1 and j, lcp[0] = lcp[n] = 0.  The text ends in its unique smallest byte, so two
    suffixes differ at or before the shorter one's terminator: no comparison reads the zeros behind the text as a match"""
    text, sa = np.asarray(text, np.uint8), np.asarray(sa, np.int64)
    n = len(text)
    K = pack_keys8(text)
    phi = np.full(n, -1, np.int64)                      # the suffix one row up
    phi[sa[1:]] = sa[:-1]
    pos = np.arange(n, dtype=np.int64)
    reducible = (pos > 0) & (phi > 0)
    reducible[reducible] = text[pos[reducible] - 1] == text[phi[reducible] - 1]
    plcp = np.zeros(n, np.int64)
    a = pos[~reducible & (phi >= 0)]
    b = phi[a]
    length = np.zeros(len(a), np.int64)
    act = np.arange(len(a))
    for _ in range(8):                                  # 64 symbols for all pairs at once; the few that go on are compared slice by slice
        x = K[a[act] + length[act]] ^ K[b[act] + length[act]]
        same = x == 0
        diff = x[~same]
        lead = np.zeros(len(diff), np.int64)            # the equal leading bytes of a window that differs
        for s in range(56, 0, -8):
            lead += (diff >> np.uint64(s)) == 0
        length[act[~same]] += lead
        act = act[same]
        length[act] += 8
    for p in act.tolist():
        length[p] = _extend(text, int(a[p]), int(b[p]), int(length[p]))
    plcp[a] = length
    anchor = np.maximum.accumulate(np.where(reducible, 0, pos))      # the last irreducible position at or before i
    plcp = plcp[anchor] - (pos - anchor)
    lcp = np.zeros(n + 1, np.int64)
    lcp[:n] = plcp[sa]
    lcp[0] = 0
    return lcp


def rounds_of(longest):
    """tests/test_gpu_sa_build.py::rounds_model"""
    rounds, h = 1, 8
    while h <= longest:
        rounds, h = rounds + 1, h * 2
    return rounds


def counter_model(text, sa):
    """{rounds, sorted, tied_after_first} of the build, from the LCP array alone"""
    lcp = lcp_array(text, sa)
    tied_to = np.maximum(lcp[:-1], lcp[1:])             # per row: the longer common prefix with a neighbour
    m, k = [], 0
    while True:
        m.append(int((tied_to >= (8 << k)).sum()))
        if m[-1] == 0:
            break
        k += 1
    return dict(rounds=1 + k, sorted=len(text) + sum(m), tied_after_first=m[0])


def doubling_simulation(text):
    """group-head prefix doubling in numpy -> (suffix array, {rounds, sorted, tied_after_first}): a rank is the first row of its group, a suffix alone in
    its group leaves the list, the first round sorts by eight bytes"""
    text = np.asarray(text, np.uint8)
    n = len(text)

    def heads(new):
        return np.maximum.accumulate(np.where(new, np.arange(len(new)), 0))

    def alone(new):
        return new & np.append(new[1:], True)

    K = pack_keys8(text)
    order = np.argsort(K, kind="stable")
    new = np.append(True, K[order][1:] != K[order][:-1])
    rank = np.empty(n, np.int64)
    rank[order] = heads(new)
    act = order[~alone(new)]
    rounds, total, tied, h = 1, n, len(act), 8
    while len(act):
        r1 = rank[act]
        r2 = np.where(act + h < n, rank[np.minimum(act + h, n - 1)], 0)
        o = np.lexsort((r2, r1))
        act, r1, r2 = act[o], r1[o], r2[o]
        new_g = np.append(True, r1[1:] != r1[:-1])
        new_s = new_g | np.append(True, r2[1:] != r2[:-1])
        rank[act] = r1 + (heads(new_s) - heads(new_g))
        rounds, total = rounds + 1, total + len(act)
        act = act[~alone(new_s)]
        h *= 2
    sa = np.empty(n, np.int64)
    sa[rank] = np.arange(n)
    return sa, dict(rounds=rounds, sorted=total, tied_after_first=tied)
