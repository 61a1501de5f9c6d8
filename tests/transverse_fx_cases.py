"""Dense problems for the transverse sweep on FIXED-POINT fields (sga_sweep_transverse_dense under option
"clf_fixed_point", csrc/sweep_transverse_fx.hip), shared by tests/test_transverse_fx_host.py and
tests/test_transverse_fx_gpu.py.  Built on the generators of tests/transverse_dense_cases.py (dc):
  quarter  J = dc.couplings(n) / 4, h zero or real-valued / 4, T0 / 4: k = 2, int32 fields, fp32 rows -- n = 24 (under a
           window), 130 (padded rows), 1100 (several chunks and super-windows), 1400 (one wave: the TAIL build);
  offgrid  J = dc.couplings(n), h = half-integers + 0.3: integer J the integer form refuses for its h -- k = 0, int8 rows,
           int32 fields;
           and n = 3200 (+-1 couplings, one wave: int8 rows of four 1-KiB chunks, the fourth streamed past the wave's first
           three -- the TAIL build over int8 rows);
  wide     J = m 2^-20, 2^23 <= |m| < 2^24, n = 300: max_i sum_j |m_ij| = 3.85e9 >= 2^31 -- k = 20, int64 fields.
Temperatures are dc.temps' ladder at the case's T0, chosen so that 10 ... 40 % of the proposals are accepted (asserted on
the reference's counts).  The reference runs (tests/transverse_reference.py over oracle.Problem(J=...)) are computed once
per case and shared."""
import functools

import numpy as np

import oracle
import transverse_dense_cases as dc
import transverse_reference as tr

SEED = (21 << 32) | 3400
NS = 3
ARITHS = dc.ARITHS
CASES = {"quarter": dict(sizes=[24, 130, 1100], kinds=["zero", "real"], bits=32, k=2, rows="float"),
         "offgrid": dict(sizes=[24, 130, 1100], kinds=["half+0.3"], bits=32, k=0, rows="int8_t"),
         "wide": dict(sizes=[300], kinds=["real"], bits=64, k=20, rows="float")}
TAIL_N = 1400  # `quarter` only, one wave: fp32 rows of six 1-KiB chunks, the sixth streamed past the wave's first five
TAIL_N_I8 = 3200  # `offgrid` only, one wave: int8 rows of four 1-KiB chunks, the fourth streamed past the wave's first three
# (+-1 couplings: the typical |dE| grows as sqrt(n) times the rms coupling -- dc's n = 1100, rms 1.58, runs at T0 = 22, which
#  gives 0.42 sqrt(3200) = 24 here)
OFFGRID_LONG_T0 = 24.0


def pgs(n):
    return dc.PG_SMALL if n <= 130 else [(2, 1), (4, 1)]


# every (case, n, h kind, P, G) the device test runs against the reference
GRID = [(c, n, kind, P, G) for c, d in CASES.items() for n in d["sizes"] for kind in d["kinds"] for P, G in pgs(n)]


def realh(n):
    return np.random.RandomState(7100 + n).uniform(-1.5, 1.5, n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def wide_couplings():
    n = 300
    rng = np.random.RandomState(4700)
    m = np.triu(rng.randint(2 ** 23, 2 ** 24, (n, n)) * (rng.randint(0, 2, (n, n)) * 2 - 1), 1).astype(np.int64)
    m = m + m.T
    assert np.abs(m).sum(axis=1).max() >= 2 ** 31  # the fields do not fit int32
    J = (m.astype(np.float64) * 2.0 ** -20).astype(np.float32)
    assert np.array_equal(J.astype(np.float64) * 2.0 ** 20, m)  # (24-bit integers: exact in fp32)
    J.setflags(write=False)
    return J


@functools.lru_cache(maxsize=None)
def couplings(case, n):
    if case == "wide":
        return wide_couplings()
    if case == "offgrid" and n == TAIL_N_I8:
        rng = np.random.RandomState(4000 + n)
        J = np.triu(rng.randint(0, 2, (n, n)) * 2 - 1, 1).astype(np.float32)
        J = J + J.T
    else:
        J = dc.couplings(n) * np.float32(0.25) if case == "quarter" else dc.couplings(n).copy()
    J.setflags(write=False)
    return J


@functools.lru_cache(maxsize=None)
def fields(case, n, kind):
    if case == "quarter":
        h = np.zeros(n, np.float32) if kind == "zero" else realh(n) * np.float32(0.25)
    elif case == "offgrid":
        half = np.random.RandomState(7000 + n).randint(-3, 4, n).astype(np.float32) / 2 if n == TAIL_N_I8 else dc.fields(n, "half")
        h = half + np.float32(0.3)
    else:
        h = realh(n) * np.float32(8)
    h = np.ascontiguousarray(h, np.float32)
    h.setflags(write=False)
    return h


def T0(case, n):
    if case == "offgrid" and n == TAIL_N_I8:
        return OFFGRID_LONG_T0
    return {"quarter": dc.SHAPE[n]["T0"] / 4, "offgrid": dc.SHAPE[n]["T0"], "wide": 85.0}[case]


def temps(case, n, P, G):
    """dc.temps' ladder at the case's T0: equal within a group, distinct between groups."""
    return np.repeat(T0(case, n) * (1.0 + 0.3 * np.arange(G)), P)


k_perp = dc.k_perp


def problem(case, n, kind):
    return oracle.Problem(J=couplings(case, n), h=fields(case, n, kind).copy())


@functools.lru_cache(maxsize=None)
def reference(case, n, kind, P, G, arith):
    """(spins, out) of NS sweeps under k_perp(G) from oracle.init_spins at SEED; shared, not to be written to."""
    S = oracle.init_spins(n, P * G, SEED)
    out = tr.sweeps(problem(case, n, kind), S, temps(case, n, P, G), NS, P, k_perp(G), arith=arith, seed=SEED)
    S.setflags(write=False)
    for v in out.values():
        v.setflags(write=False)
    return S, out


def acceptance(n, out):
    """Accepted share of the proposals, over all slices."""
    return float(out["n_accepted"].sum()) / float(out["n_accepted"].size * NS * n)
