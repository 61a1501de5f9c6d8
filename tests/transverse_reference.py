"""The transverse sweep (sga_sweep_transverse, include/sga.h) in plain Python over the oracle: the specification.

The local replicas are G groups of P slices.  Sweep kk is two half-sweeps: the slices with even p = (replica0 + r) % P
move while the odd ones stand still, then the odd ones.  A moving slice performs the n updates of the production stream
(oracle.stream_site / oracle.stream_u at (seed, replica0 + r, sweep0 + kk, t)); the update at site i is
oracle.metropolis_update on a problem whose h[i] is the fp32 h_eff = h_i + k (s_up[i] + s_dn[i]); on accept the tracked
energy moves by the classical dE -- the dE of the same update on a scratch copy at T = inf (always accepted) with the
classical h.  After both half-sweeps every slice's best follows where its energy is lower.
"""
import copy

import numpy as np

import oracle


def update(work, h0, s, up, dn, i, k, T, u, arith=oracle.ARITH_F64):
    """One update of slice s (int8 [n], in place) at site i under neighbours up / dn and coupling k with the uniform u.
    work: a problem whose field vector work.h may be written (left equal to h0).  Returns (accepted, classical dE)."""
    a = int(up[i]) + int(dn[i])
    work.h[i] = np.float32(h0[i]) + np.float32(k) * np.float32(a)  # fp32: an exact product, one rounding
    accepted, _ = oracle.metropolis_update(work, s, i, T, u, arith=arith)
    work.h[i] = h0[i]
    if not accepted:
        return False, 0.0
    scratch = s.copy()
    scratch[i] = -scratch[i]  # as before the flip
    took, dE = oracle.metropolis_update(work, scratch, i, np.inf, u, arith=arith)
    assert took
    return True, dE


def field_problem(prob):
    """(work, h0): the same couplings under a field vector of its own, and the classical fields."""
    work = copy.copy(prob)
    work.h = prob.h.copy()
    return work, prob.h.copy()


def sweeps(prob, spins, temps, n_sweeps, n_slices, k_perp, arith=oracle.ARITH_F64, seed=0, sweep0=0, replica0=0, energy=None,
           best_energy=None, best_spins=None):
    """In place on spins [R, n] int8 (the LOCAL replicas).  temps [R]; k_perp a scalar, [n_sweeps] or [n_sweeps, G].
    Returns dict(energy, best_energy, best_spins, n_accepted)."""
    R, n = spins.shape
    assert spins.dtype == np.int8 and spins.flags.c_contiguous and n == prob.n
    P = int(n_slices)
    assert P >= 2 and P % 2 == 0 and R % P == 0 and replica0 % P == 0
    G = R // P
    k = np.asarray(k_perp, np.float32)
    k = np.broadcast_to(k[:, None] if k.ndim == 1 else k, (n_sweeps, G))
    T = np.broadcast_to(np.asarray(temps, np.float64), (R,))
    E = np.asarray([oracle.energy(prob, spins[r]) for r in range(R)], np.float64) if energy is None else np.array(energy, np.float64)
    bestE = E.copy() if best_energy is None else np.array(best_energy, np.float64)
    bestS = spins.copy() if best_spins is None else np.array(best_spins, np.int8)
    nacc = np.zeros(R, np.int64)
    work, h0 = field_problem(prob)
    for kk in range(n_sweeps):
        for parity in (0, 1):
            start = spins.copy()  # the neighbour slices as they stand at the start of the half-sweep
            for r in range(R):
                p = (replica0 + r) % P
                if p % 2 != parity:
                    continue
                g = r // P
                up, dn = start[g * P + (p + 1) % P], start[g * P + (p - 1) % P]
                s = spins[r]
                for t in range(n):
                    i = oracle.stream_site(seed, replica0 + r, sweep0 + kk, t, n)
                    u = oracle.stream_u(seed, replica0 + r, sweep0 + kk, t)
                    accepted, dE = update(work, h0, s, up, dn, i, k[kk, g], T[r], u, arith)
                    if accepted:
                        E[r] += dE
                        nacc[r] += 1
        lower = E < bestE
        bestE[lower] = E[lower]
        bestS[lower] = spins[lower]
    return dict(energy=E, best_energy=bestE, best_spins=bestS, n_accepted=nacc)


def effective_energy(prob, spins, n_slices, k):
    """H_eff of one group [P, n] at coupling k: sum_p E_cl(s_p) - k sum_p sum_i s_p[i] s_{p+1}[i] (P = 2: both neighbours
    are the same slice, the bond counted twice)."""
    P = int(n_slices)
    cl = sum(oracle.energy(prob, spins[p]) for p in range(P))
    inter = sum(float(np.dot(spins[p].astype(np.int64), spins[(p + 1) % P].astype(np.int64))) for p in range(P))
    return cl - float(k) * inter
