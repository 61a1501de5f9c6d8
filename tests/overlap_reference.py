"""Spin and link overlaps between pairs of replicas (sga_get_pair_overlaps / sga_accumulate_ladder_overlaps /
sga_get_link_count, csrc/pair_overlaps.hip) in plain numpy.  Everything is an integer count, so the engine is held to
these with np.array_equal.  For a pair (a, b): x_i = [s_a[i] != s_b[i]]; a link is a stored entry (i, j) whose value is
not +-0 with j != i and 0 <= j < n, both triangles as stored.  Shared by tests/test_pair_overlaps_host.py and
tests/test_pair_overlaps_gpu.py."""
import numpy as np


def dist(s_a, s_b):
    """d: the sites where the two configurations differ (n q_ab = n - 2 d)."""
    return int(np.count_nonzero(np.asarray(s_a) != np.asarray(s_b)))


def links(rowptr, colidx, val):
    """(i, j) of every link, in storage order."""
    rowptr, colidx, val = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64), np.asarray(val)
    n = len(rowptr) - 1
    i = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    j = colidx[:len(i)]
    keep = (val[:len(i)] != 0) & (j != i) & (j >= 0) & (j < n)  # (-0.0 != 0 is False: a stored -0 is no link)
    return i[keep], j[keep]


def link_count(rowptr, colidx, val):
    """L: the number of links, a constant of the problem."""
    return int(len(links(rowptr, colidx, val)[0]))


def broken(rowptr, colidx, val, s_a, s_b):
    """b: the links whose two ends differ in x (L q_l = L - 2 b)."""
    x = np.asarray(s_a) != np.asarray(s_b)
    i, j = links(rowptr, colidx, val)
    return int(np.count_nonzero(x[i] != x[j]))


def accumulate(hist_q, hist_l, slot_to_rep, L, graph, S, slot_lo=0, slot_hi=None, q_shift=0, l_shift=0):
    """What one sga_accumulate_ladder_overlaps call adds, in place: hist_q [n_ladders / 2, slots, bins_q] and hist_l
    (or None) [.., bins_l] as integer arrays, slot_to_rep the slot map (n_ladders rows of L global ids), S the spins."""
    slot_to_rep = np.asarray(slot_to_rep).reshape(-1, L)
    hi = L if slot_hi is None else slot_hi
    for c in range(slot_to_rep.shape[0] // 2):
        for s in range(slot_lo, hi):
            a, b = S[slot_to_rep[2 * c, s]], S[slot_to_rep[2 * c + 1, s]]
            hist_q[c, s - slot_lo, min(dist(a, b) >> q_shift, hist_q.shape[2] - 1)] += 1
            if hist_l is not None:
                hist_l[c, s - slot_lo, min(broken(*graph, a, b) >> l_shift, hist_l.shape[2] - 1)] += 1


def lds_bytes(n, with_links):
    """sga_replicas.h, pair_overlap_lds_bytes: 64 bytes, and with links a bitmap of ceil(n / 32) words behind them."""
    return 64 + (4 * ((n + 31) // 32) if with_links else 0)
