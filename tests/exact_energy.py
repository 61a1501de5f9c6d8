"""Exact reference for the from-scratch energy  E = -1/2 s.(J s) - h.s  and the rounding chain the engine
documents for it (include/sga.h, sga_recompute_energies; the reference's IsingModel.compute_energy):

    mv_i = fp32(S_i),  S_i = sum_j J_ij s_j        (torch.mv: one fp32 result per row)
    X = sum_i mv_i s_i,  Y = sum_i h_i s_i          (fp64)
    E = -1/2 fp32(X) - fp32(Y)                      (fp64)

Every fp32 value is dyadic, so S_i, X and Y are computed here exactly with Python integers scaled by a power of
two.  `contract_energy` applies the chain's roundings to the exact sums: what every kernel must return whenever
its row sums and its fp64 sums X and Y are exact (integer and narrow-range dyadic problems).  `energy_bound` is a
proven bound on |E - E*| for any order of the sums, for the problems where they are not.

Problems are dense float32 matrices, CSR triples (rowptr, colidx, val) -- the ragged batches and the TSP rows of
encoders.tsp_csr among them -- and float32 h.
"""
from fractions import Fraction

import numpy as np

F32_MANT = 24
F32_MIN_EXP = -149  # lowest set bit of an fp32 (subnormal)
U53 = 2.0 ** -53    # fp64 unit roundoff
U24 = 2.0 ** -24    # fp32 unit roundoff


def _split(v):
    """float32 values -> (int64 mantissas, exponents): v = m * 2**e exactly, m = 0 for zeros."""
    m, e = np.frexp(np.asarray(v, np.float32).astype(np.float64))
    return (m * 2.0 ** F32_MANT).astype(np.int64), (e - F32_MANT).astype(np.int64)


def _round_f32(num, exp):
    """fp32 nearest-even rounding of the exact value num * 2**exp (Python ints), as a Python float."""
    if num == 0:
        return 0.0
    neg, a = num < 0, abs(num)
    # keep 24 significant bits, but never a bit below 2^-149 (subnormals)
    drop = max(a.bit_length() - F32_MANT, F32_MIN_EXP - exp)
    if drop > 0:
        q, rem = a >> drop, a & ((1 << drop) - 1)
        half = 1 << (drop - 1)
        if rem > half or (rem == half and q & 1):
            q += 1
        a, exp = q, exp + drop
    f = float(Fraction(a) * (Fraction(2) ** exp)) if exp < 0 else float(a << exp)
    if f > float(np.finfo(np.float32).max):
        f = float("inf")
    return -f if neg else f


def _exact_sum(vals, signs):
    """sum_k vals_k * signs_k exactly, vals float32-representable: (num, exp) with value num * 2**exp."""
    m, e = _split(vals)
    nz = m != 0
    if not nz.any():
        return 0, 0
    lo = int(e[nz].min())
    total = 0
    for mk, ek, sk in zip(m[nz].tolist(), e[nz].tolist(), np.asarray(signs)[nz].tolist()):
        total += (mk * sk) << (ek - lo)
    return total, lo


class Rows:
    """The rows of J as (row index, column, value) triples, with the exact row sums for a spin vector."""

    def __init__(self, J=None, csr=None):
        if J is not None:
            J = np.asarray(J, np.float32)
            self.n = J.shape[0]
            r, c = np.nonzero(J)
            self.rows, self.cols, self.vals = r.astype(np.int64), c.astype(np.int64), J[r, c]
        else:
            rp, ci, v = (np.asarray(x) for x in csr)
            self.n = len(rp) - 1
            self.rows = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(rp).astype(np.int64))
            self.cols, self.vals = ci.astype(np.int64), np.asarray(v, np.float32)
            keep = self.vals != 0
            self.rows, self.cols, self.vals = self.rows[keep], self.cols[keep], self.vals[keep]
        self.row_len = np.bincount(self.rows, minlength=self.n).astype(np.int64)
        self.abs_row = np.bincount(self.rows, weights=np.abs(self.vals.astype(np.float64)), minlength=self.n)
        self.m, self.e = _split(self.vals)

    def row_sums(self, s):
        """Exact S_i = sum_j J_ij s_j: (list of Python ints, exponent) with S_i = num_i * 2**exp."""
        s = np.asarray(s, np.int64)
        if self.vals.size == 0:
            return [0] * self.n, 0
        lo = int(self.e.min())
        # windows of exponents whose shifted mantissas add up in int64 without overflow
        width = max(1, 62 - F32_MANT - int(max(1, self.row_len.max())).bit_length())
        sums = [0] * self.n
        hi = int(self.e.max())
        for w0 in range(lo, hi + 1, width):
            sel = (self.e >= w0) & (self.e < w0 + width)
            if not sel.any():
                continue
            t = np.zeros(self.vals.size, np.int64)
            t[sel] = (self.m[sel] << (self.e[sel] - w0)) * s[self.cols[sel]]
            cs = np.concatenate([[0], np.cumsum(t)])
            ends = np.cumsum(self.row_len)
            part = cs[ends] - cs[ends - self.row_len]
            shift = w0 - lo
            for i in np.nonzero(part)[0].tolist():
                sums[i] += int(part[i]) << shift
        return sums, lo


def _as_rows(J=None, csr=None, rows=None):
    return rows if rows is not None else Rows(J=J, csr=csr)


def _spin_rows(s):
    s = np.asarray(s)
    return (s[None, :] if s.ndim == 1 else s), s.ndim == 1


def exact_parts(s, h, J=None, csr=None, rows=None):
    """For one spin vector: exact row sums S (Fractions), mv = fp32(S), exact X = sum mv s, Y = sum h s and the
    exact energy E* = -1/2 sum S s - sum h s (all as Fractions, mv as floats)."""
    R = _as_rows(J, csr, rows)
    s = np.asarray(s, np.int64)
    nums, ex = R.row_sums(s)
    scale = Fraction(2) ** ex
    mv = np.asarray([_round_f32(v, ex) for v in nums], np.float64)
    xs, xe = _exact_sum(mv.astype(np.float32), s)
    ys, ye = _exact_sum(np.asarray(h, np.float32), s)
    sx = sum(v * int(si) for v, si in zip(nums, s.tolist()))
    X, Y = Fraction(xs) * Fraction(2) ** xe, Fraction(ys) * Fraction(2) ** ye
    E = -Fraction(sx) * scale / 2 - Y
    return {"S": [Fraction(v) * scale for v in nums], "mv": mv, "X": X, "Y": Y,
            "X_num": (xs, xe), "Y_num": (ys, ye), "E": E}


def contract_energy(s, h, J=None, csr=None, rows=None):
    """The documented chain on exact sums: mv_i = fp32(S_i), E = -1/2 fp32(X) - fp32(Y) (fp64), X and Y exact.
    s: [n] or [R, n]; returns a float or an array of R floats."""
    R = _as_rows(J, csr, rows)
    S, one = _spin_rows(s)
    out = []
    cache = {}
    for row in S:
        key = np.asarray(row, np.int8).tobytes()
        if key not in cache:
            p = exact_parts(row, h, rows=R)
            fx, fy = _round_f32(*p["X_num"]), _round_f32(*p["Y_num"])
            cache[key] = -0.5 * fx + (-fy)
        out.append(cache[key])
    return out[0] if one else np.asarray(out)


def exact_energy(s, h, J=None, csr=None, rows=None):
    """E* = -1/2 s.(J s) - h.s exactly (Fraction; [R] list for [R, n] spins)."""
    R = _as_rows(J, csr, rows)
    S, one = _spin_rows(s)
    out = [exact_parts(row, h, rows=R)["E"] for row in S]
    return out[0] if one else out


def _gamma(k):
    k = float(max(int(k), 1))
    return k * U53 / (1.0 - k * U53)


def energy_bound(s, h, J=None, csr=None, rows=None):
    """A proven bound on |E - E*| for any implementation of the chain whatever the order of its sums:
    each row sum carries its fp64 summation error (gamma_len * sum_j |J_ij|) and one fp32 ulp; X and Y their fp64
    summation errors over n terms and one fp32 rounding; the last fp64 addition one rounding.  Returns
    (E* as a float, bound); [R] lists of both for [R, n] spins."""
    R = _as_rows(J, csr, rows)
    S, one = _spin_rows(s)
    h64 = np.abs(np.asarray(h, np.float32).astype(np.float64))
    g_n = _gamma(R.n)
    outE, outB = [], []
    for row in S:
        p = exact_parts(row, h, rows=R)
        absS = np.asarray([abs(float(v)) for v in p["S"]])
        d_row = np.asarray([_gamma(k) for k in R.row_len.tolist()]) * R.abs_row      # fp64 row sum error
        e_row = d_row + 2.0 * U24 * (absS + d_row)                                    # + one fp32 ulp
        sum_abs_mv = float(np.sum(absS + e_row))
        dX = float(np.sum(e_row)) + g_n * sum_abs_mv                                   # |X^ - X*|, X* = sum S s
        Xs = abs(float(sum(v * int(si) for v, si in zip(p["S"], np.asarray(row).tolist()))))
        dX += U24 * (Xs + dX)                                                           # fp32(X)
        dY = g_n * float(np.sum(h64))
        dY += U24 * (abs(float(p["Y"])) + dY)                                           # fp32(Y)
        Ef = float(p["E"])
        b = 0.5 * dX + dY
        b += U53 * (abs(Ef) + b)                                                        # the fp64 addition
        outE.append(Ef)
        outB.append(b * (1.0 + 2.0 ** -20) + 2.0 ** -140)                               # margin for the float bound
    return (outE[0], outB[0]) if one else (outE, outB)


# ---------------------------------------------------------------------------------------------------------------
# problem classes the tests draw from
# ---------------------------------------------------------------------------------------------------------------
def witness_dense(n=64, i=0, j=9, k=17, l=30, p=40, q=41):
    """The +-2^60 cancellation: J[i][j] = 2^60, J[k][l] = -2^60, J[p][q] = 1 (symmetric), h = 0; at all spins +1
    E* = -1, and an fp64 sum of X that meets 2^61 before the small term loses it."""
    J = np.zeros((n, n), np.float32)
    for a, b, v in ((i, j, 2.0 ** 60), (k, l, -2.0 ** 60), (p, q, 1.0)):
        J[a, b] = J[b, a] = v
    return J, np.zeros(n, np.float32)


def sym(A):
    A = np.triu(np.asarray(A, np.float32), 1)
    return (A + A.T).astype(np.float32)


def dense_to_csr(J):
    J = np.asarray(J, np.float32)
    n = J.shape[0]
    nz = J != 0
    rowptr = np.concatenate([[0], np.cumsum(nz.sum(1))]).astype(np.int64)
    r, c = np.nonzero(nz)
    return rowptr, c.astype(np.int32), J[r, c].astype(np.float32)


def f64_inexact_x(n=1024, e_hi=20, seed=0):
    """A problem of the f64-exact class (every J within 52 - ceil(log2 n) binary places of every other, so each row
    sum is exact in fp64 in any order) whose X = sum_i mv_i s_i is NOT exact in fp64.  Odd rows of the first half
    couple to each other with +2^e_hi, odd rows of the second half with -2^e_hi, even rows to each other with tiny
    values at the class's lowest binary place.  At all spins +1 the two large groups cancel in X, but a partial sum
    of X in row order meets ~(n/4)^2 2^e_hi on the way, and the tiny row sums lose bits to it: how many depends on
    the order of the additions.  Returns (J, h) with h = 0; n a multiple of 4."""
    carry = max(1, (n - 1).bit_length())
    e_lo = e_hi - (52 - carry) + 1
    rng = np.random.RandomState(seed)
    i = np.arange(n)
    plus, minus, tiny = (i % 2 == 1) & (i < n // 2), (i % 2 == 1) & (i >= n // 2), i % 2 == 0
    A = np.zeros((n, n), np.float64)
    A[np.ix_(plus, plus)] = 2.0 ** e_hi
    A[np.ix_(minus, minus)] = -2.0 ** e_hi
    A[np.ix_(tiny, tiny)] = rng.randint(-7, 8, (int(tiny.sum()),) * 2) * 2.0 ** e_lo
    return sym(A), np.zeros(n, np.float32)


def canonical_x(mv, s, block_rows=None):
    """X = sum_i mv_i s_i in the engine's canonical energy order (sga_kernels.h, energy_block_rows), fp64."""
    n = len(mv)
    B = block_rows or max(8, (n + 255) // 256)
    terms = [float(m) * float(v) for m, v in zip(np.asarray(mv, np.float64), np.asarray(s))]
    X = 0.0
    for b0 in range(0, n, B):
        c = []
        for l in range(4):
            acc = 0.0
            for i in range(b0 + l, min(n, b0 + B), 4):
                acc += terms[i]
            c.append(acc)
        X += (c[0] + c[1]) + (c[2] + c[3])
    return X


def sequential_x(mv, s):
    """X summed row by row from 0 (the order of the CSR all-replica pass when every row is its own group)."""
    X = 0.0
    for m, v in zip(np.asarray(mv, np.float64), np.asarray(s)):
        X += float(m) * float(v)
    return X
