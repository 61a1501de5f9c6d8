"""World-line cluster updates (sga_worldline_clusters, include/sga.h) in plain Python over the oracle: the specification.

The local replicas are G groups of P slices, as in transverse_reference.py.  Per sweep kk the sites go in typewriter
order; at site i slice p (global id q_p = replica0 + g P + p) takes the Philox block at counter (i, round + kk, q_p, 4)
under the seed: word 0 draws the bond towards slice (p + 1) % P against thr = floor(p_bond 2^24), word 1 is the uniform
u_p.  Bonds between equal spins cut the ring of slices into segments; a segment with head f, size m and spin sigma flips
under dE = 2 sigma (A + m h_i), A the sum of the members' integer row sums, by the oracle's fp64 Metropolis rule with
u_f; a flipped slice's tracked energy moves by its own classical dE.  After the n sites every slice's best follows
where its energy is lower.
"""
import numpy as np

import oracle

DOMAIN_WORLDLINE = 4


def threshold(p_bond):
    """floor(p 2^24), in double: p = 1 gives 2^24, above every 24-bit draw."""
    return int(np.floor(np.float64(p_bond) * 16777216.0))


def draws(seed, i, rnd, q):
    """(24 bits of word 0, u from word 1 as fp32) of slice q's block at site i in round rnd."""
    w = oracle.philox((i, rnd & 0xFFFFFFFF, q, DOMAIN_WORLDLINE), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return int(w[0]) >> 8, np.float32(int(w[1]) >> 8) * np.float32(2.0 ** -24)


def segments(column, bonds):
    """The segments of one site's ring of P slices.  column: the P spins; bonds[p]: the draw of the bond from slice p to
    slice (p + 1) % P succeeded -- the bond is active iff the two spins are equal as well.  Returns [(head, members)] by
    ascending head; members run cyclically from the head up to the slice before the next head."""
    P = len(column)
    active = [bool(bonds[p]) and column[p] == column[(p + 1) % P] for p in range(P)]
    heads = [p for p in range(P) if not active[(p - 1) % P]]
    if not heads:
        return [(0, list(range(P)))]
    out = []
    for a, f in enumerate(heads):
        nxt = heads[(a + 1) % len(heads)]
        m = (nxt - f) % P or P
        out.append((f, [(f + d) % P for d in range(m)]))
    return out


def row_sum(prob, s, i):
    """sum_j J_ij s[j] as an exact integer (integer couplings)."""
    lo, hi = int(prob.rowptr[i]), int(prob.rowptr[i + 1])
    v = prob.val[lo:hi].astype(np.int64)
    assert np.array_equal(v, prob.val[lo:hi])
    return int(np.dot(v, s[prob.colidx[lo:hi]].astype(np.int64)))


def decide(dE, T, u):
    """The fp64 Metropolis rule: dE <= 0, or u < expf((float)(-dE / T))."""
    if dE <= 0.0:
        return True
    with np.errstate(divide="ignore", over="ignore"):
        x = np.float32(np.float64(-dE) / np.float64(T))
    return float(u) < oracle.expf(x)


def site_update(prob, S, i, T, thr, bits, us):
    """One site of one group, in place on S [P, n] int8.  bits[p], us[p]: slice p's 24 bond bits and its uniform.
    Returns the segments' records [dict(head, members, A, dE, flip)] and dE_slice [P] (0 where the slice stays)."""
    P = S.shape[0]
    column = [int(S[p, i]) for p in range(P)]
    dots = [row_sum(prob, S[p], i) for p in range(P)]
    h = np.float64(prob.h[i])
    records, moved = [], np.zeros(P, np.float64)
    for f, members in segments(column, [bits[p] < thr for p in range(P)]):
        sigma = column[f]
        assert all(column[p] == sigma for p in members)
        A = sum(dots[p] for p in members)
        dE = 2.0 * np.float64(sigma) * (np.float64(A) + np.float64(len(members)) * h)
        flip = decide(dE, T, us[f])
        records.append(dict(head=f, members=members, A=A, dE=float(dE), flip=flip))
        if flip:
            for p in members:
                S[p, i] = -sigma
                moved[p] = 2.0 * np.float64(sigma) * (np.float64(dots[p]) + h)
    return records, moved


def sweeps(prob, spins, temps, n_sweeps, n_slices, p_bond, seed=0, round=0, replica0=0, energy=None, best_energy=None,
           best_spins=None):
    """In place on spins [R, n] int8 (the LOCAL replicas).  temps [R]; p_bond a scalar, [n_sweeps] or [n_sweeps, G].
    Returns dict(energy, best_energy, best_spins, stats [G, 3]: segments formed, segments flipped, slice spins flipped)."""
    R, n = spins.shape
    assert spins.dtype == np.int8 and spins.flags.c_contiguous and n == prob.n
    P = int(n_slices)
    assert 2 <= P <= 64 and R % P == 0 and replica0 % P == 0
    G = R // P
    pb = np.asarray(p_bond, np.float64)
    pb = np.broadcast_to(pb[:, None] if pb.ndim == 1 else pb, (n_sweeps, G))
    T = np.broadcast_to(np.asarray(temps, np.float64), (R,))
    E = np.asarray([oracle.energy(prob, spins[r]) for r in range(R)], np.float64) if energy is None else np.array(energy, np.float64)
    bestE = E.copy() if best_energy is None else np.array(best_energy, np.float64)
    bestS = spins.copy() if best_spins is None else np.array(best_spins, np.int8)
    stats = np.zeros((G, 3), np.int64)
    for kk in range(n_sweeps):
        for g in range(G):
            grp = spins[g * P:(g + 1) * P]
            thr = threshold(pb[kk, g])
            for i in range(n):
                d = [draws(seed, i, round + kk, replica0 + g * P + p) for p in range(P)]
                records, moved = site_update(prob, grp, i, T[g * P], thr, [x[0] for x in d], [x[1] for x in d])
                E[g * P:(g + 1) * P] += moved
                stats[g] += (len(records), sum(r["flip"] for r in records), sum(len(r["members"]) for r in records if r["flip"]))
        lower = E < bestE
        bestE[lower] = E[lower]
        bestS[lower] = spins[lower]
    return dict(energy=E, best_energy=bestE, best_spins=bestS, stats=stats)
