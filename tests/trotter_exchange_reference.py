"""The broken time links and the exchange between Trotter groups along the transverse field (sga_get_time_links,
sga_exchange_transverse; include/sga.h) in plain Python over oracle.philox and oracle.exp: the specification.

The local replicas are G groups of P slices, slice p of group g in row g P + p, the slices of a group a ring.
B_g = sum_p sum_i [s_{gP+p}[i] != s_{gP+next(p)}[i]].  One exchange round takes the pairs (a, a + 1) with a % 2 == parity:

    beta_g = 1.0 / T[gP]            E_g = energy[gP] + ... + energy[gP+P-1], left to right
    x = (beta_a - beta_b) * (E_a - E_b) + (2.0 * (beta_a * k_a - beta_b * k_b)) * (B_a - B_b)     (fp64, k from fp32)
    swap iff u < (1.0 if not x < 0.0 else exp(x)),  u the 53 bits of words 0, 1 of Philox at counter (0, round, a, 8)

-- the log ratio of the weights exp(-beta H_eff), H_eff = E - k (n P - 2 B).  A pair with a T that is not positive and
finite is left alone.  On a swap the two groups trade spin rows and tracked energies slice by slice; then every slice's
best follows where its energy is lower."""
import numpy as np

import oracle

DOMAIN_TROTTER_EXCHANGE = 8


def time_links(S, P):
    """int64 [G] of spins S [G P, n]."""
    S = np.asarray(S)
    R = S.shape[0]
    assert P >= 2 and R % P == 0
    out = np.zeros(R // P, np.int64)
    for g in range(R // P):
        for p in range(P):
            out[g] += int(np.count_nonzero(S[g * P + p] != S[g * P + (p + 1) % P]))
    return out


def u53(w0, w1):
    return ((int(w0) >> 5) * 67108864.0 + (int(w1) >> 6)) * 2.0 ** -53


def draw(seed, round_, a):
    w = oracle.philox((0, round_ & 0xFFFFFFFF, a, DOMAIN_TROTTER_EXCHANGE), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return u53(w[0], w[1])


def pairs(G, parity):
    return [(a, a + 1) for a in range(parity, G - 1, 2)]


def decide(E, T, k, B, P, parity, seed, round_):
    """E, T [G P]; k, B [G].  Returns [dict(a, b, x, prob, u, swap)] for every pair of the round; a pair whose T is not
    positive and finite: x = prob = u = None, swap False."""
    E, T = np.asarray(E, np.float64), np.asarray(T, np.float64)
    k = np.asarray(k, np.float32)
    G = len(B)
    assert E.shape == (G * P,) and T.shape == (G * P,) and k.shape == (G,)
    out = []
    for a, b in pairs(G, parity):
        Ta, Tb = T[a * P], T[b * P]
        if not (Ta > 0.0 and np.isfinite(Ta) and Tb > 0.0 and np.isfinite(Tb)):
            out.append(dict(a=a, b=b, x=None, prob=None, u=None, swap=False))
            continue
        beta_a, beta_b = np.float64(1.0) / Ta, np.float64(1.0) / Tb
        Ea, Eb = E[a * P], E[b * P]
        for p in range(1, P):
            Ea = Ea + E[a * P + p]
            Eb = Eb + E[b * P + p]
        t1 = (beta_a - beta_b) * (Ea - Eb)
        c = beta_a * np.float64(k[a]) - beta_b * np.float64(k[b])
        t2 = (np.float64(2.0) * c) * np.float64(int(B[a]) - int(B[b]))
        x = float(t1 + t2)
        prob = 1.0 if not x < 0.0 else oracle.exp(x)
        u = draw(seed, round_, a)
        out.append(dict(a=a, b=b, x=x, prob=prob, u=u, swap=bool(u < prob)))
    return out


def apply(S, E, bestE, bestS, T, k, P, parity, seed, round_):
    """One round on copies of the state.  Returns dict(spins, energy, best_energy, best_spins, accepted int32 [G],
    links int64 [G] (before the exchange), decisions)."""
    S, E = np.array(S, np.int8), np.array(E, np.float64)
    bestE, bestS = np.array(bestE, np.float64), np.array(bestS, np.int8)
    G = S.shape[0] // P
    B = time_links(S, P)
    decisions = decide(E, T, k, B, P, parity, seed, round_)
    accepted = np.zeros(G, np.int32)
    for d in decisions:
        if d["swap"]:
            a, b = d["a"], d["b"]
            ra, rb = slice(a * P, (a + 1) * P), slice(b * P, (b + 1) * P)
            S[ra], S[rb] = S[rb].copy(), S[ra].copy()
            E[ra], E[rb] = E[rb].copy(), E[ra].copy()
            accepted[a] = accepted[b] = 1
    lower = E < bestE
    bestE[lower] = E[lower]
    bestS[lower] = S[lower]
    return dict(spins=S, energy=E, best_energy=bestE, best_spins=bestS, accepted=accepted, links=B, decisions=decisions)
