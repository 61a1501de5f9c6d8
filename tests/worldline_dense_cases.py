"""Cases for world-line cluster updates on dense couplings (sga_worldline_clusters_dense), shared by
tests/test_worldline_dense_host.py and tests/test_worldline_dense_gpu.py.  The problems are those of
tests/transverse_dense_cases.py (full symmetric integer matrices, zero diagonal; h zero, integer or half-integer), at the
four sizes at which the kernel takes another path --
  n = 24    shorter than one block of 32 sites,
  n = 130   several blocks, a tail of 2 sites, padded rows,
  n = 300   int32 fields,
  n = 1100  several 1-KiB chunks of a row per wave, 34 blocks and a tail --
and the specification is tests/worldline_reference.py run on the same couplings as full CSR rows
(transverse_dense_cases.problem(n, kind, as_csr=True)).  Two starts, 2 sweeps each:
  "independent"  oracle.init_spins; p_bond per sweep and group cycles through {0.6, 0, 1, 0.3};
  "correlated"   every slice a copy of one random row with 15 % of its spins flipped independently, p_bond = 0.9,
                 round = 0xFFFFFFFF, so that the second sweep's round wraps to 0.
Every case holds the conditions of check_counts on the reference's own counts.  At P = 2 a flipped segment of the
correlated start averages about 1.5 slices -- a pair or a single slice, nothing else exists -- which is the bound itself,
so there the start is the first draw (START_DRAW) at which the reference's count lies above it for all three kinds of h.
The reference runs are computed once per case and shared; nobody writes to them."""
import functools

import numpy as np

import oracle
import transverse_dense_cases as dc
import worldline_reference as wr

SEED = (32 << 32) | 1207
NS = 2
SMALL, LARGE = [24, 130], [300, 1100]
PG_SMALL = [(2, 3), (3, 1), (4, 3), (32, 1), (34, 1), (64, 1)]
PG_LARGE = [(2, 1), (4, 1)]
GRID = [(n, P, G) for n in SMALL for P, G in PG_SMALL] + [(n, P, G) for n in LARGE for P, G in PG_LARGE]
H_KINDS = dc.H_KINDS
STARTS = ["independent", "correlated"]
P_CYCLE = np.asarray([0.6, 0.0, 1.0, 0.3])
WRAP_ROUND = 0xFFFFFFFF
START_DRAW = {(24, 2): 3, (24, 3): 1, (300, 2): 1}  # (n, P): which draw of the correlated start is taken (else the first)


def p_bond(start, G, ns=NS):
    """float64 [ns, G]."""
    if start == "independent":
        return P_CYCLE[(np.arange(ns)[:, None] + np.arange(G)[None, :]) % 4].astype(np.float64)
    return np.full((ns, G), 0.9, np.float64)


def round0(start):
    return 0 if start == "independent" else WRAP_ROUND


def start_spins(start, n, P, G):
    """int8 [P G, n], a fresh array."""
    if start == "independent":
        return oracle.init_spins(n, P * G, SEED)
    rng = np.random.RandomState(9000 + 64 * n + P + 100000 * START_DRAW.get((n, P), 0))
    S = np.empty((P * G, n), np.int8)
    for g in range(G):
        row = (rng.randint(0, 2, n) * 2 - 1).astype(np.int8)
        S[g * P:(g + 1) * P] = np.where(rng.rand(P, n) < 0.15, -row, row)
    return S


@functools.lru_cache(maxsize=None)
def reference(n, kind, P, G, start):
    """(S0, S, out): the start, the spins after NS sweeps and worldline_reference.sweeps' record (energy, best_energy,
    best_spins, stats, and energy0: the energies of the start)."""
    S0 = start_spins(start, n, P, G)
    S = S0.copy()
    prob = dc.problem(n, kind, as_csr=True)
    out = wr.sweeps(prob, S, dc.temps(n, P, G), NS, P, p_bond(start, G), seed=SEED, round=round0(start))
    out["energy0"] = np.asarray([oracle.energy(prob, r) for r in S0], np.float64)
    for a in (S0, S, *out.values()):
        a.setflags(write=False)
    return S0, S, out


def check_counts(out, start):
    """The conditions on the reference's own counts: a test cannot pass on a sweep in which nothing moves."""
    formed, flipped, spins = (float(x) for x in out["stats"].sum(axis=0))
    assert 0.15 <= flipped / formed <= 0.55, (flipped, formed)
    if start == "correlated":
        assert spins / flipped >= 1.5, (spins, flipped)
