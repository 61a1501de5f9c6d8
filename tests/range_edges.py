"""Instances that sit exactly at the limits of the exact-integer sweep forms' number ranges, and a group-sum reference
that never materialises J (test infrastructure of tests/test_range_edges_host.py and tests/test_range_edges_gpu.py; the
window section at the end: of tests/test_window_range_edges_host.py and tests/test_window_range_edges_gpu.py).

Saturating instances: a gauge xi in {+-1}^n, J_ij = a_ij xi_i xi_j with integer a_ij = a_ji >= 0 and a zero diagonal,
h_i = b_i xi_i with b_i >= 0.  In state s = xi every s_i F_i equals its row's bound sum_j a_ij + b_i; row 0's bound is
EXACTLY the limit L (in units of 1/scale), every other row lies strictly below at its own value, falling linearly to
about L/16 so that moves of many sizes occur and the colder replicas both accept and refuse.  Replica 0 starts at xi,
replica 1 at -xi, replica 2 at xi with site 0 flipped, the others from oracle.init_spins; temperatures per replica
cycle through {0, L/8, L/2, 2L, inf} (in units of the field, L/scale).

Twins: L is the last value a form admits, L+ the first it does not -- by the CODE's condition (csrc/sga_problem.cpp):
"scale * m < 32768", "m * scale < 16777216", "mj < 32768", "max_size >= (1 << 15)": all on integers, so L+ = L + 1."""
import functools

import numpy as np

import oracle
from exact_energy import _exact_sum, _round_f32

INF = float("inf")
GAUGE_SEED = 7


def gauge(n):
    return (np.random.RandomState(GAUGE_SEED).randint(0, 2, n) * 2 - 1).astype(np.int64)


def row_bounds(L, n):
    """t_0 = L; t_1 = L - 1 (one unit below: a proposal within one coupling of the limit); then strictly decreasing to
    about L/16.  Units of 1/scale."""
    t = np.empty(n, np.int64)
    t[0] = L
    t[1:] = L - 1 - (np.arange(n - 1, dtype=np.int64) * (L - 1 - L // 16)) // max(n - 2, 1)
    assert (np.diff(t) < 0).all() or L < 16 * n
    return t


def _couplings(r, jmax=None, mask=None):
    """Symmetric non-negative integers a_ij ~ r_i r_j / S with sum_j a_ij <= r_i in every row (floors only lose)."""
    m = np.ones((r.size, r.size), bool) if mask is None else mask.copy()
    np.fill_diagonal(m, False)
    S = int((m * r[None, :]).sum(1).max())
    a = (np.outer(r, r) // S) * m
    if jmax is not None:
        a = np.minimum(a, jmax)
    assert (a == a.T).all() and (a.sum(1) <= r).all()
    return a


def dense_n(L, scale, jmax):
    """The smallest n >= 67, no multiple of 64, at which no coupling of the instance needs clipping to jmax: the couplings
    then carry (nearly) the whole bound and the largest one equals jmax (asserted in the host tests).  |J| <= 127 and
    L = 32767: n = 483, not the ~260 that rows all near L would need -- the rows fall to L/16, not L/2, because only then
    does the T = L/8 replica accept anything in two sweeps (at L/2 its best move has exp(-8)); lower rows carry less, so
    more of them are needed to fill row 0."""
    n = 67
    while True:
        if n % 64:
            r = row_bounds(L, n) // scale
            if jmax is None or int(r[0]) * int(r[1]) // int(r[1:].sum()) <= jmax:
                return n
        n += 1


def saturating_dense(L, scale=1, jmax=None, n=None):
    """(J fp32 [n, n], h fp32 [n], xi int8 [n]): row 0's bound scale * (sum_j |J_0j| + |h_0|) == L exactly."""
    n = n or dense_n(L, scale, jmax)
    xi = gauge(n)
    t = row_bounds(L, n)
    a = _couplings(t // scale, jmax)
    b2 = t - scale * a.sum(1)          # units of 1/scale: what the couplings leave of the bound goes to the field
    assert (b2 >= 0).all() and (scale == 1 or (b2 % 2).any())  # scale 2: some h is a half-integer
    J = (a * np.outer(xi, xi)).astype(np.float32)
    h = (b2 * xi / float(scale)).astype(np.float32)
    assert scale * (np.abs(J).astype(np.float64).sum(1) + np.abs(h)).max() == L
    return J, h, xi.astype(np.int8)


def single_coupling_dense(L=32767, n=131):
    """Row 0 is ONE coupling of L - 1 (to site 1) plus |h_0| = 1: an accept at site 1 moves site 0's field across the
    whole range, +L -> -(L - 2).  Row 1 holds that coupling alone (bound L - 1); sites 2.. form a saturating instance
    of their own at a limit below."""
    J = np.zeros((n, n), np.float32)
    h = np.zeros(n, np.float32)
    Js, hs, xs = saturating_dense(L - 767, 1, None, n - 2)
    xi = np.concatenate([gauge(2), xs.astype(np.int64)])
    J[2:, 2:], h[2:] = Js, hs
    J[0, 1] = J[1, 0] = float(L - 1) * xi[0] * xi[1]
    h[0] = float(xi[0])
    return J, h, xi.astype(np.int8)


def flat_dense(amp, n, spike=None):
    """Every off-diagonal |J_ij| = amp in the gauge (h_0 = 1 breaks the tie of the rows); `spike`: J_01 raised to it."""
    xi = gauge(n)
    a = np.full((n, n), amp, np.int64)
    np.fill_diagonal(a, 0)
    if spike is not None:
        a[0, 1] = a[1, 0] = spike
    h = np.zeros(n, np.float32)
    h[0] = float(xi[0])
    return (a * np.outer(xi, xi)).astype(np.float32), h, xi.astype(np.int8)


def saturating_csr(L, n=333, half_width=40, h_extra=3 << 15):
    """Ring-banded sparse instance: max_i sum_j |J_ij| == L exactly (row 0; the deficit of the band construction is put
    on the coupling to site n - 1, whose own row stays far below).  |h_i| = h_extra + i: several times 2^15, so only the
    dynamic part J s fits 16 bits.  Returns (csr, h, xi, J dense fp32)."""
    xi = gauge(n)
    i = np.arange(n)
    d = np.abs(i[:, None] - i[None, :])
    mask = np.minimum(d, n - d) <= half_width
    t = row_bounds(L, n)
    a = _couplings(t, None, mask)
    a[0, n - 1] += L - a[0].sum()
    a[n - 1, 0] = a[0, n - 1]
    rs = a.sum(1)
    assert rs[0] == L and (rs[1:] < L).all()
    J = (a * np.outer(xi, xi)).astype(np.float32)
    h = ((h_extra + i) * xi).astype(np.float32)
    return csr_of(J), h, xi.astype(np.int8), J


def table_edge_csr(L, n=333, half_width=40):
    """The accept table's edge (sga_engine.cpp, table_covers: table_scale * csr_row_abs_max <= table_m): a banded sparse
    instance whose row 0 has sum_j |J_0j| + |h_0| == L exactly, row 1 L - 1.  L = 2048: table_m = 2048 covers every move;
    L = 2049: table_m is still 2048, the move k = s_0 F_0 = 2049 = table_m + 1 lies beyond it and k = 2048 = table_m
    (site 1) is its last entry.  Integer h.  Returns (csr, h, xi, J dense fp32)."""
    xi = gauge(n)
    i = np.arange(n)
    d = np.abs(i[:, None] - i[None, :])
    t = row_bounds(L, n)
    a = _couplings(t, None, np.minimum(d, n - d) <= half_width)
    b = t - a.sum(1)
    J = (a * np.outer(xi, xi)).astype(np.float32)
    h = (b * xi).astype(np.float32)
    assert (np.abs(J).astype(np.float64).sum(1) + np.abs(h)).max() == L
    return csr_of(J), h, xi.astype(np.int8), J


# Fixed-point fields (option "clf_fixed_point"): int32 while ldexp(m, k) * (1 + 2^-20) < 2^31, m the FP32 ROUNDING of
# max_i sum_j |J_ij| (csrc/sga_problem.cpp).  Couplings in multiples of 2^-8 (k = 8), bounds in those units.  The code's
# condition is more conservative than "2^k bound < 2^31" twice over: the margin admits fp32 values up to 2^31 - 2048
# only ((2^31 - 2048)(1 + 2^-20) = 2^31 - 2^-9; the next fp32 value, 2^31 - 1920, is refused), and the fp32 rounding
# (ulp 128 there, ties to even) maps every exact bound up to 2^31 - 1984 onto 2^31 - 2048.  So the largest bound the
# code's condition admits is 2^31 - 1984 and the smallest it refuses 2^31 - 1983.
FX_K = 8
FX_IN, FX_OUT = (1 << 31) - 1984, (1 << 31) - 1983


def fixed_point_bits(M):
    """The width the set-time scan gives fields of bound M (units of 2^-FX_K)."""
    m = np.float32(M / 2.0 ** FX_K)
    return 32 if np.ldexp(np.float64(m), FX_K) * (1.0 + 2.0 ** -20) < 2.0 ** 31 else 64


def fixed_point_dense(M, n=349):
    """Dyadic couplings a_ij 2^-8 in the gauge, h = 0: 2^8 sum_j |J_0j| == M exactly, so D_0 = 2^8 (J s)_0 = +-M at
    s = +-xi.  Every a_ij < 2^24 (an fp32 value), some odd (k = 8).  Returns (J, h, xi)."""
    xi = gauge(n)
    a = _couplings(row_bounds(M, n))
    a[0, n - 1] += M - a[0].sum()
    a[n - 1, 0] = a[0, n - 1]
    rs = a.sum(1)
    assert rs[0] == M and (rs[1:] < M).all() and a.max() < (1 << 24) and (a % 2).any() and (a + np.eye(n, dtype=np.int64) > 0).all()
    J = (a * np.outer(xi, xi) / 2.0 ** FX_K).astype(np.float32)
    assert np.array_equal(J.astype(np.float64) * 2.0 ** FX_K, a * np.outer(xi, xi))
    return J, np.zeros(n, np.float32), xi.astype(np.int8)


def fixed_point_traits(J, csr):
    """sga_set_dense / sga_set_csr under option "clf_fixed_point" for these instances (f64-exact class, no accept table)."""
    M = int((np.abs(J).astype(np.float64).sum(1) * 2.0 ** FX_K).max())
    base = dict(n=J.shape[0], table_m=0, clf_bits=fixed_point_bits(M), options={"clf_fixed_point": 1})
    if csr:
        nnz = int(np.count_nonzero(J))
        return dict(base, kind=1, acc=2, clf_ok=1, nnz=nnz, layout_entries=nnz, max_row_len=int((J != 0).sum(1).max()))
    return dict(base, kind=0, storage=1, acc=1, clf_ok=0)


def packed_csr(spike=None, n=400, half_width=150):
    """A degree-300 ring graph, every |J_ij| = 127 in the gauge (the largest value a packed entry holds), h_0 = +-1;
    `spike`: J_01 raised to it.  Returns (csr, h, xi, J dense fp32)."""
    J, h, xi = flat_dense(127, n, spike)
    i = np.arange(n)
    d = np.abs(i[:, None] - i[None, :])
    J = (J * (np.minimum(d, n - d) <= half_width)).astype(np.float32)
    assert ((J != 0).sum(1) == 2 * half_width).all()
    return csr_of(J), h, xi, J


def packed_traits(csr):
    """The route query of the long-row bit-spin form (options force_csr_bits, two waves) for this graph."""
    rp, col, val = csr
    n = rp.size - 1
    slots = int(((np.diff(rp) + 63) // 64 * 64).sum())
    return dict(kind=1, n=n, nnz=val.size, max_row_len=int(np.diff(rp).max()), layout_entries=slots, slotted=1, acc=0,
                table_m=2048, tune_waves=2, R_local=5, options={"force_csr_bits": 1},
                packed_ok=int(float(np.abs(val).max()) <= 127.0))


def csr_of(J):
    n = J.shape[0]
    rowptr = np.concatenate([[0], np.cumsum((J != 0).sum(1))]).astype(np.int32)
    col = np.concatenate([np.nonzero(J[i])[0] for i in range(n)] + [np.zeros(0, int)]).astype(np.int32)
    val = np.concatenate([J[i][J[i] != 0] for i in range(n)] + [np.zeros(0)]).astype(np.float32)
    return rowptr, col, val


def start_spins(xi, R, seed):
    """Replica 0 at xi, 1 at -xi, 2 at xi with site 0 flipped, the others the oracle's random spins."""
    s = oracle.init_spins(xi.size, R, seed)
    s[0] = xi
    if R > 1:
        s[1] = -xi
    if R > 2:
        s[2] = xi
        s[2, 0] = -xi[0]
    return s


def temperatures(R, unit):
    """{0, L/8, L/2, 2L, inf} cycled over the replicas; `unit` = L / scale, the field at the limit."""
    return np.asarray([[0.0, unit / 8.0, unit / 2.0, 2.0 * unit, INF][r % 5] for r in range(R)])


def proposals(J, h, s0, temps, n_sweeps, seed, replay_u=None):
    """The oracle's traced run from s0 plus the dE of EVERY proposal (the oracle traces 0 for a refused one): the chain
    is followed along the oracle's accept trace with the exact fields F = J s + h (integers and halves: exact in fp64).
    `replay_u` [R, n_sweeps * n]: the sequential order on these recorded uniforms (update t proposes site t) instead of
    the Philox stream's random sites.  Returns (oracle result, proposed dE [R, n_sweeps * n], final spins)."""
    n, R = J.shape[0], s0.shape[0]
    s = s0.copy()
    if replay_u is None:
        ref = oracle.sweeps(oracle.Problem(J=J, h=h), s, temps, n_sweeps, seed=seed, trace=True)
    else:
        ref = oracle.sweeps(oracle.Problem(J=J, h=h), s, temps, n_sweeps, site_mode=oracle.SITE_SEQUENTIAL, replay_u=replay_u,
                            seed=seed, trace=True)
    J64, out = J.astype(np.float64), np.zeros((R, n_sweeps * n))
    for r in range(R):
        v = s0[r].astype(np.float64)
        F = J64 @ v + h
        for k in range(n_sweeps):
            for t in range(n):
                i = oracle.stream_site(seed, r, k, t, n) if replay_u is None else t
                out[r, k * n + t] = 2.0 * v[i] * F[i]
                if ref["accept_trace"][r, k * n + t]:
                    assert out[r, k * n + t] == ref["dE_trace"][r, k * n + t]
                    v[i] = -v[i]
                    F += 2.0 * v[i] * J64[:, i]
        assert np.array_equal(v, s[r])
    return ref, out, s


# ---------------------------------------------------------------------------------------------------------------------
# what the set-time scans of csrc/sga_problem.cpp find (a host mirror: the route pins need no device)
# ---------------------------------------------------------------------------------------------------------------------
def dense_traits(J, h, storage="f32"):
    """sga_set_dense's classification: clf_ok, clf_bits, clf_scale, table_m, acc, storage (sga_route_query fields)."""
    m = float(np.float32((np.abs(J).astype(np.float64).sum(1) + np.abs(h)).max()))
    j_int, h_int = bool((J == np.rint(J)).all()), bool((h == np.rint(h)).all())
    h_half = bool((2 * h == np.rint(2 * h)).all())
    fits_i8 = j_int and float(np.abs(J).max()) <= 127
    i8 = storage == "i8" or (storage == "auto" and fits_i8)
    scale = 1 if h_int else 2
    return dict(kind=0, n=J.shape[0], storage=2 if i8 else 1,
                acc=0 if i8 or (j_int and m < 16777216.0) else 1,
                table_m=int(min(m, 2048.0)) if (j_int and h_int and 1.0 <= m < 16777216.0) else 0,
                clf_scale=scale, clf_ok=int(j_int and h_half and m * scale < 16777216.0),
                clf_bits=16 if m * scale < 32768.0 else 32)


def csr_traits(csr, h):
    """sga_set_csr's classification of an integer problem with integer h (symmetric, sorted, zero diagonal)."""
    rp, col, val = csr
    n = rp.size - 1
    row = np.repeat(np.arange(n), np.diff(rp))
    mj = np.bincount(row, weights=np.abs(val).astype(np.float64), minlength=n)
    m = float(np.float32((mj + np.abs(h)).max()))
    table_m = int(min(m, 2048.0)) if 1.0 <= m < 16777216.0 else 0
    return dict(kind=1, n=n, nnz=val.size, max_row_len=int(np.diff(rp).max()), layout_entries=val.size,
                acc=0 if table_m else 1, table_m=table_m, table_scale=1,
                clf_ok=int(table_m > 0 and float(np.float32(mj.max())) < 32768.0))


# ---------------------------------------------------------------------------------------------------------------------
# couplings as a sum of complete graphs on groups (+ a stored remainder): the oracle's chain without J
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def streams(n, R, n_sweeps, seed):
    """(sites int [R, n_sweeps * n], uniforms float [R, n_sweeps * n]) of the oracle's production stream."""
    sites = np.empty((R, n_sweeps * n), np.int64)
    us = np.empty((R, n_sweeps * n), np.float64)
    for r in range(R):
        for k in range(n_sweeps):
            for t in range(n):
                sites[r, k * n + t] = oracle.stream_site(seed, r, k, t, n)
                us[r, k * n + t] = oracle.stream_u(seed, r, k, t)
    return sites, us


class GroupProblem:
    """Groups (member_ptr, members, coeff), fields h and an optional remainder (rowptr, colidx, val); coefficients and
    remainder values are integer multiples of one 2^-k (k found here), so every row sum is a Python integer of that unit."""

    def __init__(self, n, member_ptr, members, coeff, h, rest=None):
        self.n, self.mp, self.mem = int(n), np.asarray(member_ptr, np.int64), np.asarray(members, np.int64)
        self.h = np.asarray(h, np.float32)
        vals = [float(c) for c in np.asarray(coeff, np.float32)] + ([float(v) for v in rest[2]] if rest is not None else [])
        k = 0
        while any(v * 2.0 ** k != np.rint(v * 2.0 ** k) for v in vals):
            k += 1
            assert k <= 30
        self.k, self.unit = k, 2.0 ** -k
        self.c = [int(np.rint(float(c) * 2.0 ** k)) for c in np.asarray(coeff, np.float32)]
        self.size = np.diff(self.mp)
        self.group_of = np.repeat(np.arange(self.size.size), self.size)       # group of every membership
        self.site_groups = [[] for _ in range(self.n)]
        for g, i in zip(self.group_of.tolist(), self.mem.tolist()):
            self.site_groups[i].append((g, self.c[g]))
        self.rest_rows = None
        if rest is not None:
            rp, ci, v = rest
            self.rest = (np.asarray(rp, np.int64), np.asarray(ci, np.int64), np.rint(np.asarray(v, np.float64) * 2.0 ** k).astype(np.int64))
            self.rest_rows = [list(zip(self.rest[1][rp[i]:rp[i + 1]].tolist(), self.rest[2][rp[i]:rp[i + 1]].tolist()))
                              for i in range(self.n)]

    def sums(self, s):
        return np.bincount(self.group_of, weights=s[self.mem].astype(np.float64), minlength=self.size.size).astype(np.int64)

    def rows(self, s):
        """row_i = sum_{g contains i} c_g (S_g - s_i) (+ sum_j R_ij s_j), int64 units of 2^-k."""
        s = np.asarray(s, np.int64)
        S = self.sums(s)
        cg = np.asarray(self.c, np.int64)[self.group_of]
        out = np.zeros(self.n, np.int64)
        np.add.at(out, self.mem, cg * (S[self.group_of] - s[self.mem]))
        if self.rest_rows is not None:
            rp, ci, v = self.rest
            np.add.at(out, np.repeat(np.arange(self.n), np.diff(rp)), v * s[ci])
        return out

    def energy(self, s):
        """From scratch by the rounding chain of tests/exact_energy.py: mv_i = fp32(row_i) (exact: the set-time bound),
        exact X = sum_i mv_i s_i and Y = sum_i h_i s_i, E = -1/2 fp32(X) - fp32(Y)."""
        s = np.asarray(s, np.int64)
        rows = self.rows(s)
        assert np.abs(rows).max() < (1 << 24)  # units of 2^-k: every mv_i is the exact row sum
        X = sum(int(a) * int(b) for a, b in zip(rows.tolist(), s.tolist()))
        return -0.5 * _round_f32(X, -self.k) + (-_round_f32(*_exact_sum(self.h, s)))

    def sweeps(self, s, temps, n_sweeps, seed):
        """oracle.sweeps(..., trace=True) on the couplings these groups stand for; in place on s [R, n] int8."""
        R, n = s.shape
        sites, us = streams(n, R, n_sweeps, seed)
        h = self.h.astype(np.float64).tolist()
        energy = np.asarray([self.energy(s[r]) for r in range(R)])
        best_energy, best_spins = energy.copy(), s.copy()
        trace = np.zeros((n_sweeps, R))
        acc_tr, dE_tr = np.zeros((R, n_sweeps * n), np.uint8), np.zeros((R, n_sweeps * n))
        n_acc = np.zeros(R, np.int64)
        for r in range(R):
            v = s[r].astype(np.int64).tolist()
            S = self.sums(s[r]).tolist()
            E, T = float(energy[r]), float(temps[r])
            for k in range(n_sweeps):
                for t in range(n):
                    idx = k * n + t
                    i = int(sites[r, idx])
                    si, row = v[i], 0
                    for g, c in self.site_groups[i]:
                        row += c * (S[g] - si)
                    if self.rest_rows is not None:
                        for j, w in self.rest_rows[i]:
                            row += w * v[j]
                    dE = 2.0 * si * (row * self.unit + h[i])
                    # oracle/sg_oracle.c, metropolis_core: dE <= 0, or u < expf(float32(-dE / T))
                    if dE <= 0.0 or (T > 0.0 and us[r, idx] < oracle.expf(-dE / T)):
                        v[i] = -si
                        for g, _ in self.site_groups[i]:
                            S[g] -= 2 * si
                        E += dE
                        acc_tr[r, idx], dE_tr[r, idx] = 1, dE
                        n_acc[r] += 1
                trace[k, r] = E
                if E < best_energy[r]:
                    best_energy[r], best_spins[r] = E, np.asarray(v, np.int8)
            s[r] = np.asarray(v, np.int8)
            energy[r] = E
        return dict(energy=energy, energy_trace=trace, n_accepted=n_acc, best_energy=best_energy, best_spins=best_spins,
                    accept_trace=acc_tr, dE_trace=dE_tr)


GROUPS_SEED, GROUPS_R, GROUPS_SWEEPS = 5, 4, 2


@functools.lru_cache(maxsize=None)
def big_group(G, big_coeff, with_rest):
    """One group of G members (sites 0 .. G - 1), behind it a 17 x 17 grid whose rows and columns are groups with
    coefficient -4, a singleton group and one site in no group; half-integer fields.  `big_coeff`: the big group's
    coefficient is the largest integer for which max_i (sum_g |c_g| (|g| - 1) + sum_j |R_ij|) < 2^24 still holds
    (computed here from the instance), else -1.  `with_rest`: a few symmetric integer pairs inside the big group.
    Returns (GroupProblem, (n, (member_ptr, members), coeff, h, rest), s0, temps)."""
    n = G + 17 * 17 + 1
    grid = G + np.arange(17 * 17).reshape(17, 17)
    groups = [np.arange(G)] + [grid[i] for i in range(17)] + [grid[:, j] for j in range(17)]
    groups[17] = groups[17][:-1]          # (the grid's last site leaves its row ...
    groups[34] = groups[34][:-1]          #  ... and its column: in no group)
    groups.append(np.asarray([G + 100]))  # a singleton; site n - 1 is the extra site in two grid groups
    groups[1] = np.append(groups[1], n - 1)
    groups[18] = np.append(groups[18], n - 1)
    rest, rest_share = None, 0
    if with_rest:
        pairs = [(0, 1, 3.0), (0, G - 1, -5.0), (1, 2, 7.0), (64, 4097, -2.0), (G // 2, G - 2, 4.0), (63, 64, 1.0)]
        ii, jj, vv = (np.asarray(x) for x in zip(*[(i, j, v) for i, j, v in pairs] + [(j, i, v) for i, j, v in pairs]))
        order = np.lexsort((jj, ii))                       # rows sorted, columns sorted inside a row
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(ii, minlength=n))])
        rest = (rowptr.astype(np.int32), jj[order].astype(np.int32), vv[order].astype(np.float32))
        rest_share = int(np.bincount(ii, weights=np.abs(vv), minlength=n).max())
    c0 = float((16777215 - rest_share) // (G - 1)) if big_coeff else -1.0
    coeff = np.asarray([c0] + [-4.0] * 34 + [-12.0], np.float32)
    h = (np.random.default_rng(5).integers(-4, 5, n) / 2.0).astype(np.float32)
    mp = np.concatenate([[0], np.cumsum([g.size for g in groups])]).astype(np.int64)
    mem = np.concatenate(groups).astype(np.int32)
    prob = GroupProblem(n, mp, mem, coeff, h, rest)
    bound = abs(c0) * (G - 1) + rest_share
    assert bound < 16777216 and (not big_coeff or (abs(c0) + 1) * (G - 1) + rest_share >= 16777216)
    s0 = oracle.init_spins(n, GROUPS_R, GROUPS_SEED)
    s0[0, :G] = 1      # the big group aligned: S_g = +G ...
    s0[1, :G] = -1     # ... and -G
    unit = abs(c0) * (G - 1)
    temps = np.asarray([0.0, 2.0 * unit, unit / 8.0, INF])
    return prob, (n, (mp, mem), coeff, h, rest), s0, temps


@functools.lru_cache(maxsize=None)
def big_group_reference(G, big_coeff, with_rest):
    prob, _, s0, temps = big_group(G, big_coeff, with_rest)
    s = s0.copy()
    out = prob.sweeps(s, temps, GROUPS_SWEEPS, GROUPS_SEED)
    out["spins"] = s
    out["scratch"] = np.asarray([prob.energy(s[r]) for r in range(s.shape[0])])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the instances by name: what both test files run
# ---------------------------------------------------------------------------------------------------------------------
# name -> (L, scale, jmax, n): L in units of 1/scale.  Twins: "..._in" is the last value the code's condition admits,
# "..._out" the first it refuses (integers: L + 1).
DENSE = {
    "i16_in": (32767, 1, 127, None), "i16_out": (32768, 1, 127, None),               # clf_bits: scale * m < 32768
    "i16h_in": (32767, 2, 127, None), "i16h_out": (32768, 2, 127, None),             # ... m = 16383.5 | 16384, scale 2
    "i24_in": ((1 << 24) - 1, 1, None, 67), "i24_out": (1 << 24, 1, None, 67),       # clf_problem / acc64: m < 2^24
    "i24h_in": ((1 << 24) - 1, 2, None, 67), "i24h_out": (1 << 24, 2, None, 67),     # ... m = 2^23 - 1/2 | 2^23, scale 2
}
# seeds at which every instance meets the input conditions of tests/test_range_edges_host.py (site 0 is proposed in
# replicas 0 and 2 before its neighbourhood moves, every finite-T replica accepts and refuses)
SEEDS = {"i16_in": 218, "i16_out": 218, "i16h_in": 44, "i16h_out": 44, "i24_in": 44, "i24_out": 44, "i24h_in": 44,
         "i24h_out": 44, "single": 1, "c16_in": 1, "c16_out": 1, "t2048": 218, "t2049": 218}
R_MAIN, SWEEPS = 5, 2


@functools.lru_cache(maxsize=None)
def dense_case(name, seed=None):
    if name == "single":
        J, h, xi = single_coupling_dense()
        L, scale = 32767, 1
    elif name.startswith("fx_"):
        L, scale = {"fx_in": FX_IN, "fx_out": FX_OUT}[name], 1 << FX_K
        J, h, xi = fixed_point_dense(L)
    else:
        L, scale, jmax, n = DENSE[name]
        J, h, xi = saturating_dense(L, scale, jmax, n)
    seed = SEEDS.get(name, 1) if seed is None else seed
    s0 = start_spins(xi, R_MAIN, seed)
    return dict(J=J, h=h, xi=xi, L=L, scale=scale, seed=seed, s0=s0, temps=temperatures(R_MAIN, L / scale), sweeps=SWEEPS)


@functools.lru_cache(maxsize=None)
def csr_case(name, seed=None):
    if name.startswith("t20"):                         # table_covers: table_scale * csr_row_abs_max <= table_m
        L = int(name[1:])
        csr, h, xi, J = table_edge_csr(L)
        unit = float(L)
    else:
        L = {"c16_in": 32767, "c16_out": 32768}[name]  # clf_csr_problem: mj < 32768
        csr, h, xi, J = saturating_csr(L)
        unit = float(L + np.abs(h).max())
    seed = SEEDS.get(name, 1) if seed is None else seed
    return dict(csr=csr, J=J, h=h, xi=xi, L=L, scale=1, seed=seed, s0=start_spins(xi, R_MAIN, seed),
                temps=temperatures(R_MAIN, unit), sweeps=SWEEPS)


def case(name):
    return csr_case(name) if name[:3] in ("c16", "t20") else dense_case(name)


@functools.lru_cache(maxsize=None)
def reference(name, rule=0, as_csr=False):
    """oracle.sweeps(trace=True) of the named instance from its explicit spins; 'spins' the final state, 'scratch' its
    from-scratch energies.  `as_csr`: a dense instance handed over as CSR (the oracle then walks its rows as CSR does)."""
    c = case(name)
    if as_csr:
        c = dict(c, csr=csr_of(c["J"]))
    prob = oracle.Problem(csr=c["csr"], h=c["h"]) if "csr" in c else oracle.Problem(J=c["J"], h=c["h"])
    s = c["s0"].copy()
    out = oracle.sweeps(prob, s, c["temps"], c["sweeps"], seed=c["seed"], trace=True, rule=rule)
    out["spins"], out["scratch"] = s, oracle.energy(prob, s)
    return out


def flat_reference(J, h, s0, temps, n_sweeps, seed, trace=False):
    prob = oracle.Problem(J=J, h=h)
    s = s0.copy()
    out = oracle.sweeps(prob, s, temps, n_sweeps, seed=seed, trace=trace, n_threads=8)
    out["spins"], out["scratch"] = s, oracle.energy(prob, s)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the window forms (tests/test_window_range_edges_{host,gpu}.py): sequential windows (csrc/sweep_dense_seq.hip) and
# row-shared windows on a binary grid (sga_classify::row_shared_grid, csrc/sweep_dense_rs.hip)
# ---------------------------------------------------------------------------------------------------------------------
def product_saturating_dense(L, n, reverse=False):
    """Integer J in the gauge, h = 0, sum_j |J_0j| == L exactly (the deficit of the construction goes on a[0, n - 1], as
    in fixed_point_dense): at s = +-xi the window-start product of row 0 is +-L itself and every partial sum along the
    row rises monotonically to it.  `reverse`: J[::-1, ::-1] with xi reversed -- the limit row is site n - 1, the last
    update of the last window, whose field has taken the corrections of every accept before it.  Returns (J, h, xi)."""
    xi = gauge(n)
    a = _couplings(row_bounds(L, n))
    a[0, n - 1] += L - a[0].sum()
    a[n - 1, 0] = a[0, n - 1]
    rs = a.sum(1)
    assert rs[0] == L and (rs[1:] < L).all() and a.max() < (1 << 24) and (a + np.eye(n, dtype=np.int64) > 0).all()
    J = (a * np.outer(xi, xi)).astype(np.float32)
    assert np.array_equal(J.astype(np.float64), a * np.outer(xi, xi))
    if reverse:
        J, xi = np.ascontiguousarray(J[::-1, ::-1]), xi[::-1]
    return J, np.zeros(n, np.float32), np.ascontiguousarray(xi).astype(np.int8)


def grid_flat(amp, k, M, n=300):
    """Couplings on the grid 2^-k under a field that carries the bound: J_ij = a_ij 2^-k xi_i xi_j with a_ij = amp off
    the diagonal, h_i = xi_i (row_bounds(M, n)_i - sum_j a_ij) 2^-k, so that s_i F_i = row_bounds_i 2^-k at s = xi and
    row 0 has 2^k (sum_j |J_0j| + |h_0|) == M exactly.  The set-time scan takes k from the lowest set bit of any J: where
    amp is even ONE coupling (sites 1, 2) is amp - 1, or the scan would find the coarser grid of amp's trailing zeros and
    a scaled maximum below amp (the twins are the code's: its k, its 2^k max |J|).  Returns (J, h, xi)."""
    xi = gauge(n)
    a = np.full((n, n), amp, np.int64)
    np.fill_diagonal(a, 0)
    if amp % 2 == 0:
        a[1, 2] = a[2, 1] = amp - 1
    t = row_bounds(M, n)
    b = t - a.sum(1)  # (negative where the couplings alone exceed the row's bound: the gauge property holds all the same)
    unit = 2.0 ** -k
    J = (a * np.outer(xi, xi) * unit).astype(np.float32)
    h = (b * xi * unit).astype(np.float32)
    assert np.array_equal(J.astype(np.float64) * 2.0 ** k, a * np.outer(xi, xi))  # the intended integers, exactly
    assert np.array_equal(h.astype(np.float64) * 2.0 ** k, b * xi)
    assert (a % 2).any() and a.max() == amp
    rows = (np.abs(J).astype(np.float64).sum(1) + np.abs(h)) * 2.0 ** k
    assert rows[0] == M and (rows[1:] < M).all() and b[0] > 0
    return J, h, xi.astype(np.int8)


def grid_verdict(J, h):
    """sga_classify::row_shared_grid as written (a host mirror of its conditions on these instances -- symmetric, zero
    diagonal, no canonical-order class; tests/test_window_range_edges_host.py holds it against the compiled classifier):
    (k, planes), planes = 0 where the verdict refuses."""
    from scan_reference import bit_span
    m = float(np.float32((np.abs(J).astype(np.float64).sum(1) + np.abs(h)).max()))
    integer = bool((J == np.rint(J)).all() and (h == np.rint(h)).all())
    if integer and 1.0 <= m < 16777216.0:
        return 0, 0  # the integer form's
    k = max(0, -bit_span(J)[1])
    scaled = float(np.abs(J).max()) * 2.0 ** k
    if k > 30 or scaled > 255.0 or not np.ldexp(m, k) * (1.0 + 2.0 ** -20) < 16777216.0:
        return 0, 0
    return k, 1 if scaled <= 1.0 else 3 if scaled <= 7.0 else 8


P24_IN, P24_OUT = (1 << 24) - 1, 1 << 24          # the integer class: m < 2^24 (acc f32, table_m > 0)
GB_IN, GB_OUT = (1 << 24) - 16, (1 << 24) - 15    # fx_bound: (2^24 - 16)(1 + 2^-20) = 2^24 - 2^-16 < 2^24 <= the next one
# name -> (L, n, reverse): product_saturating_dense
PRODUCT = {
    "p24_in_n67": (P24_IN, 67, False), "p24_out_n67": (P24_OUT, 67, False),
    "p24_in_n579": (P24_IN, 579, False), "p24_out_n579": (P24_OUT, 579, False),
    "p24_in_n579_reversed": (P24_IN, 579, True),
}
# name -> (amp, k, M, planes the verdict gives (0: refused), the sequential product's matrix cores): grid_flat, n = 300
GRID = {
    "bound_in": (7, 3, GB_IN, 3, "i8"), "bound_out": (7, 3, GB_OUT, 0, None),
    "amp1": (1, 3, 1 << 20, 1, "i8"), "amp2": (2, 3, 1 << 20, 3, "i8"),
    "amp7": (7, 3, 1 << 20, 3, "i8"), "amp8": (8, 3, 1 << 20, 8, "f32"),
    "amp255": (255, 3, 1 << 20, 8, "f32"), "amp256": (256, 3, 1 << 20, 0, None),
    "k30_amp7": (7, 30, GB_IN, 3, "i8"), "k31_amp7": (7, 31, GB_IN, 0, None),
    "k30_amp255": (255, 30, GB_IN, 8, "f32"), "k31_amp255": (255, 31, GB_IN, 0, None),
}
FLAT = {"flat127": None, "flat127_spike128": 128}   # flat_dense(127, 131, spike): the int8 copy's |m| <= 127
WINDOW_SEQ = list(PRODUCT) + ["i24_in", "i24_out"] + list(FLAT) + list(GRID)
WINDOW_RANDOM = list(GRID)
# Seeds at which every instance meets the input conditions of tests/test_window_range_edges_host.py.  Sequential order:
# the seed of the random start spins and of the recorded uniforms; random sites: the Philox seed too -- at 218 replica 2
# proposes site 0 in its first update, before anything has moved that field.
WINDOW_SEED_SEQ, WINDOW_SEED_RANDOM = 44, 218


def recorded_u(R, n_sweeps, n, seed):
    """One array of uniforms for the engine and the oracle alike (sequential order: update t of sweep k is site t)."""
    return np.random.RandomState(seed).rand(R, n_sweeps * n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def window_case(name, order="seq"):
    """The named instance with its start spins, temperatures and, in sequential order, its recorded uniforms "u"."""
    limit_row = 0
    if name in PRODUCT:
        L, n, reverse = PRODUCT[name]
        J, h, xi = product_saturating_dense(L, n, reverse)
        scale, limit_row = 1, n - 1 if reverse else 0
    elif name in DENSE:
        L, scale, jmax, n = DENSE[name]
        J, h, xi = saturating_dense(L, scale, jmax, n)
    elif name in FLAT:
        J, h, xi = flat_dense(127, 131, FLAT[name])
        L, scale = int((np.abs(J).astype(np.float64).sum(1) + np.abs(h)).max()), 1
    else:
        amp, k, M = GRID[name][:3]
        J, h, xi = grid_flat(amp, k, M)
        L, scale = M, 2.0 ** k
    seed = WINDOW_SEED_SEQ if order == "seq" else WINDOW_SEED_RANDOM
    s0 = start_spins(xi[::-1] if limit_row else xi, R_MAIN, seed)
    if limit_row:  # the mirror image of the forward instance's start: replica 2 has the limit row flipped
        s0 = np.ascontiguousarray(s0[:, ::-1])
    c = dict(J=J, h=h, xi=xi, L=L, scale=scale, seed=seed, s0=s0, temps=temperatures(R_MAIN, L / scale), sweeps=SWEEPS,
             limit_row=limit_row, order=order)
    if order == "seq":
        c["u"] = recorded_u(R_MAIN, SWEEPS, J.shape[0], seed)
    return c


@functools.lru_cache(maxsize=None)
def window_reference(name, order="seq", rule=0, arith=None):
    """oracle.sweeps of the named instance in the given order; 'spins' the final state, 'scratch' its from-scratch
    energies."""
    c = window_case(name, order)
    prob = oracle.Problem(J=c["J"], h=c["h"])
    s = c["s0"].copy()
    kw = dict(site_mode=oracle.SITE_SEQUENTIAL, replay_u=c["u"]) if order == "seq" else {}
    out = oracle.sweeps(prob, s, c["temps"], c["sweeps"], seed=c["seed"], rule=rule,
                        arith=oracle.ARITH_F64 if arith is None else arith, n_threads=5, **kw)
    out["spins"], out["scratch"] = s, oracle.energy(prob, s)
    return out
