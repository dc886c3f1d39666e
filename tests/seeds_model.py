"""Test infrastructure: plain-Python restatements of RowBowt::get_seeds_greedy (reference include/rowbowt.hpp:191-215),
get_seeds_greedy_w_sample (:222-256), locate_from_longest_seed's choice (:669-677) and find_range_w_toehold_chkpnts
(:575-606) on the oracle's primitives.  The loops are the reference's, line by line, on Oracle.LF; the toehold is not
restated (no LF_w_loc here): a seed is a fresh search from the full range with k = first_k, so the toehold after a
successful step at q[s] of the seed ending at ei is Oracle.find_range_w_toehold(q[s:ei])'s, and a checkpoint after the step
at q[s] carries Oracle.find_range_w_toehold(q[s:])'s.  Records are (lo, hi, qstart, qend, ssamp)."""
MAXU = (1 << 64) - 1


def _has_tsa(o):
    return bool(o.L.orc_has_tsa(o.h))


def seeds_greedy(o, q, min_length, w_sample=True):
    """-> [(lo, hi, qstart, qend, ssamp)] in the reference's order (the rightmost seed first)"""
    q = bytes(q)
    m = len(q)
    full = (0, o.n - 1)                                # full_range(), :115-118
    if w_sample and not _has_tsa(o):                         # :225
        return []
    out = []
    rng = prev = full                                  # :193-194 / :227-228
    pk_of = None                                       # pk = -1 (:231); else (s, ei): the last successful step was at q[s] of the seed ending at ei
    ei = m                                             # :195 / :232

    def pk():
        if not w_sample:
            return 0                                   # (the three-argument LFData leaves ssamp unset, :148-152: 0 here)
        if pk_of is None:
            return MAXU
        lo, hi, k = o.find_range_w_toehold(q[pk_of[0]:pk_of[1]])
        assert hi >= lo
        return k

    for i in range(m):                                 # :196 / :233
        rng = o.LF(rng[0], rng[1], q[m - i - 1])       # :197 / :235
        if rng[1] < rng[0]:                            # :198 / :236
            if ei - (m - i) >= min_length:             # :199 / :237
                out.append((prev[0], prev[1], m - i, ei, pk()))
            rng = prev = full                          # :204-205 / :243-245 (k = first_k; pk stays)
            ei = m - i - 1                             # :206 / :246
        else:
            prev = rng                                 # :208 / :248
            pk_of = (m - i - 1, ei)                    # :249
    if not w_sample or ei >= min_length:               # :211 (always) / :252
        out.append((prev[0], prev[1], 0, ei, pk()))
    return out


def longest_seed(seeds):
    """locate_from_longest_seed's choice (:669-677): the first seed of strictly greatest length; None when the list is empty or
    holds zero-length seeds only (best_range stays the default LFData: no locations)"""
    best, max_length = None, 0
    for rec in seeds:
        if rec[3] - rec[2] > max_length:
            max_length, best = rec[3] - rec[2], rec
    return best


def chkpnt_count(m, wsize):
    """records of a read of m symbols that occurs: floor((m - 1) / wsize) inside the loop, the final one when (m - 1) % wsize
    != 0 -- m - 1 in 64-bit wrapping arithmetic (an empty read: no step, the final record alone)"""
    m1 = (m - 1) & MAXU
    return (m1 // wsize if m else 0) + (1 if m1 % wsize else 0)


def toehold_chkpnts(o, q, wsize):
    """-> [(lo, hi, qstart, qend, ssamp)] (rowbowt.hpp:575-606)"""
    q = bytes(q)
    assert wsize > 0                                   # (the reference computes % 0)
    if not _has_tsa(o):                                      # :579
        return []
    m = len(q)
    window_ei = m                                      # :581
    rn = (0, o.n - 1)                                  # :583
    ss = o.last_run_sample()                           # :584
    out = []
    for i in range(m):                                 # :585
        rn = o.LF(rn[0], rn[1], q[m - i - 1])          # :586
        if rn[1] < rn[0]:                              # :587-590
            return []
        if window_ei - (m - i) >= wsize:               # :592
            lo, hi, ss = o.find_range_w_toehold(q[m - i - 1:])
            assert (lo, hi) == rn
            out.append((rn[0], rn[1], m - i, window_ei, ss))   # :593-595
            window_ei = m - i                          # :596
    if rn[1] >= rn[0] and ((m - 1) & MAXU) % wsize != 0:   # :599
        if m:
            lo, hi, ss = o.find_range_w_toehold(q)
            assert (lo, hi) == rn
        out.append((rn[0], rn[1], 0, m, ss))           # :600-602
    return out
