"""The exchange cases shared by tests/test_trotter_exchange_gpu.py: the 6 x 6 x 6 lattice of tests/test_transverse_gpu.py
(n = 216, CSR rows) as G groups of P = 4 slices, two transverse sweeps from oracle.init_spins under a k ladder, then one
exchange round -- all of it from the plain-Python references, computed once per case and shared.

Two ladders.  "k": equal T and couplings k_g = 1 + 0.02 g, close enough that 2 beta (k_a - k_b)(B_a - B_b) is of order one
-- swaps at prob < 1 and refusals both occur.  "T": unequal temperatures as well, T_g = 1.5 + 0.7 g, where the classical
term (beta_a - beta_b)(E_a - E_b) joins in.  coverage() counts, over the whole grid, the swaps at prob < 1 and the
refusals the reference shows: the GPU file asserts both are there."""
import functools

import numpy as np

import oracle
import transverse_reference as tr
import trotter_exchange_reference as xr
from test_transverse_gpu import shape

SEED = (33 << 32) | 3300
NAME, P, NS = "lattice6", 4, 2
GROUPS, PARITIES, LADDERS = [1, 2, 3, 4], [0, 1], ["k", "T"]
ROUND = 11


def k_ladder(G):
    return (1.0 + 0.02 * np.arange(G)).astype(np.float32)


def temps(G, ladder):
    return np.repeat(1.5 + (0.7 * np.arange(G) if ladder == "T" else np.zeros(G)), P)


@functools.lru_cache(maxsize=None)
def before(G, ladder):
    """(spins, out) after NS transverse sweeps at k_ladder(G); shared, not to be written to."""
    g, h = shape(NAME)
    prob = oracle.Problem(csr=g, h=h)
    S = oracle.init_spins(prob.n, P * G, SEED)
    out = tr.sweeps(prob, S, temps(G, ladder), NS, P, np.repeat(k_ladder(G)[None, :], NS, axis=0), seed=SEED)
    S.setflags(write=False)
    for v in out.values():
        v.setflags(write=False)
    return S, out


@functools.lru_cache(maxsize=None)
def after(G, ladder, parity):
    S, out = before(G, ladder)
    return xr.apply(S, out["energy"], out["best_energy"], out["best_spins"], temps(G, ladder), k_ladder(G), P, parity, SEED, ROUND)


def coverage():
    """(swaps at prob < 1, refusals, swaps at prob = 1) over GROUPS x PARITIES x LADDERS."""
    partial = refused = sure = 0
    for G in GROUPS:
        for ladder in LADDERS:
            for parity in PARITIES:
                for d in after(G, ladder, parity)["decisions"]:
                    partial += d["swap"] and d["prob"] < 1.0
                    sure += d["swap"] and d["prob"] == 1.0
                    refused += not d["swap"]
    return partial, refused, sure
