"""Dense problems for the transverse sweep on dense couplings (sga_sweep_transverse_dense), shared by
tests/test_transverse_dense_host.py and tests/test_transverse_dense_gpu.py: full symmetric integer matrices with a zero
diagonal, every off-diagonal entry non-zero, at the four sizes at which the kernel takes another path --
  n = 24    fewer updates than one window of 128,
  n = 130   just over one window, rows padded,
  n = 300   100 <= |J| <= 127: max_i sum_j |J_ij| >= 2^15, the fields are int32,
  n = 1100  more than one 1-KiB chunk of an int8 row, several super-windows --
with h zero, integer or half-integer, and temperatures at which 10 ... 40 % of the proposals are accepted (asserted on the
reference's counts), so that every window is evaluated again after an accept.  The reference runs
(tests/transverse_reference.py over oracle.Problem(J=...)) are computed once per case and shared."""
import functools

import numpy as np

import oracle
import transverse_reference as tr

SEED = (20 << 32) | 2506
NS = 3
SIZES = [24, 130, 300, 1100]
SMALL, LARGE = [24, 130], [300, 1100]
PG_SMALL = [(2, 1), (2, 3), (4, 1), (4, 3), (6, 1), (6, 3)]
PG_LARGE = [(2, 1), (4, 1)]
H_KINDS = ["zero", "int", "half"]
ARITHS = [oracle.ARITH_F64, oracle.ARITH_F32]
# |J| in [lo, amp]; T0: the first group's temperature, ~ the typical |dE| of a proposal
SHAPE = {24: dict(lo=1, amp=3, T0=4.0), 130: dict(lo=1, amp=3, T0=9.0), 300: dict(lo=100, amp=127, T0=800.0),
         1100: dict(lo=1, amp=2, T0=22.0),
         1400: dict(lo=1, amp=2, T0=25.0)}  # (not in SIZES: fp32 rows of six 1-KiB chunks, streamed past a wave's first five)


@functools.lru_cache(maxsize=None)
def couplings(n):
    """float32 [n, n]: symmetric, zero diagonal, every other entry a non-zero integer in [-amp, amp]."""
    p = SHAPE[n]
    rng = np.random.RandomState(4000 + n)
    J = np.triu(rng.randint(p["lo"], p["amp"] + 1, (n, n)) * (rng.randint(0, 2, (n, n)) * 2 - 1), 1).astype(np.float32)
    J = J + J.T
    J.setflags(write=False)
    return J


@functools.lru_cache(maxsize=None)
def fields(n, kind):
    rng = np.random.RandomState(7000 + n)
    h = {"zero": np.zeros(n), "int": rng.randint(-2, 3, n), "half": rng.randint(-3, 4, n) / 2.0}[kind].astype(np.float32)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def csr(n):
    """The same couplings as CSR: every row holds its n - 1 off-diagonal entries, columns ascending."""
    J = couplings(n)
    off = ~np.eye(n, dtype=bool)
    rowptr = (np.arange(n + 1) * (n - 1)).astype(np.int32)
    col = np.tile(np.arange(n, dtype=np.int32), (n, 1))[off]
    return rowptr, col, J[off].astype(np.float32)


def temps(n, P, G):
    return np.repeat(SHAPE[n]["T0"] * (1.0 + 0.3 * np.arange(G)), P)  # equal within a group, distinct between groups


def k_perp(G, ns=NS):
    """A different k per sweep and per group, out of {0.25, 5, -1}."""
    vals = np.asarray([0.25, 5.0, -1.0], np.float32)
    return vals[(np.arange(ns)[:, None] + np.arange(G)[None, :]) % 3]


def problem(n, kind, as_csr=False):
    return oracle.Problem(csr=csr(n), h=fields(n, kind).copy()) if as_csr else oracle.Problem(J=couplings(n), h=fields(n, kind).copy())


@functools.lru_cache(maxsize=None)
def reference(n, kind, P, G, arith, as_csr=False):
    """(spins, out) of NS sweeps under k_perp(G) from oracle.init_spins at SEED; shared, not to be written to."""
    S = oracle.init_spins(n, P * G, SEED)
    out = tr.sweeps(problem(n, kind, as_csr), S, temps(n, P, G), NS, P, k_perp(G), arith=arith, seed=SEED)
    S.setflags(write=False)
    for v in out.values():
        v.setflags(write=False)
    return S, out


def acceptance(n, out):
    """Accepted share of the proposals, over all slices."""
    return float(out["n_accepted"].sum()) / float(out["n_accepted"].size * NS * n)
