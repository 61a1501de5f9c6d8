"""Class-resolved overlaps between pairs of replicas (sga_get_class_overlaps / sga_accumulate_ladder_class_overlaps,
csrc/class_overlaps.hip) in plain numpy.  Everything is an integer count, so the engine is held to these with
np.array_equal.  For a pair (a, b): x_i = [s_a[i] != s_b[i]]; a class map gives site i the class classes[m][i], and a
value outside [0, n_classes) is no class; D[m][c] = the differing sites of class c.  Shared by
tests/test_class_overlaps_host.py and tests/test_class_overlaps_gpu.py."""
import numpy as np

LDS_BUDGET = 160 * 1024 - 256  # CLUSTER_LDS_BUDGET
MAX_MC = LDS_BUDGET // 4       # one copy of the counters fills the budget: 40 896
MAX_MC_4 = LDS_BUDGET // 16    # four copies fit: 10 224


def maps(classes):
    cl = np.asarray(classes)
    return cl.reshape(1, -1) if cl.ndim == 1 else cl


def class_dist(s_a, s_b, classes, n_classes):
    """D[m][c], int32 [n_maps, n_classes]: np.bincount over the differing sites.  Sites past the map's row (ld > n has
    none; a row longer than the spins is cut) do not exist."""
    cl = maps(classes)
    n = len(s_a)
    x = np.asarray(s_a) != np.asarray(s_b)
    out = np.zeros((cl.shape[0], n_classes), np.int32)
    for m in range(cl.shape[0]):
        c = cl[m, :n][x]
        c = c[(c >= 0) & (c < n_classes)]
        out[m] = np.bincount(c, minlength=n_classes)
    return out


def pair_form(S, pairs, classes, n_classes):
    """int32 [count, n_maps, n_classes] of sga_get_class_overlaps."""
    cl = maps(classes)
    out = np.zeros((len(pairs), cl.shape[0], n_classes), np.int32)
    for k, (a, b) in enumerate(pairs):
        out[k] = class_dist(S[a], S[b], cl, n_classes)
    return out


def accumulate(sum1, sum2, slot_to_rep, L, S, classes, n_classes, slot_lo=0, slot_hi=None):
    """What one sga_accumulate_ladder_class_overlaps call adds, in place: sum1 [n_ladders / 2, slots, n_maps, C] and sum2
    (or None) [.., C, C] as uint64 arrays, slot_to_rep the slot map (n_ladders rows of L global ids), S the spins."""
    slot_to_rep = np.asarray(slot_to_rep).reshape(-1, L)
    hi = L if slot_hi is None else slot_hi
    for c in range(slot_to_rep.shape[0] // 2):
        for s in range(slot_lo, hi):
            D = class_dist(S[slot_to_rep[2 * c, s]], S[slot_to_rep[2 * c + 1, s]], classes, n_classes).astype(np.uint64)
            sum1[c, s - slot_lo] += D
            if sum2 is not None:
                sum2[c, s - slot_lo] += D[:, :, None] * D[:, None, :]


def copies(mc):
    """sga_replicas.h, class_overlap_copies: a copy of the counters for each of the four waves where four fit."""
    return 4 if mc <= MAX_MC_4 else 1


def lds_bytes(mc):
    """sga_replicas.h, class_overlap_lds_bytes: the counters, 4 bytes each, nothing else."""
    return 4 * copies(mc) * mc
