"""What the set-time scans of the problem setters must find (AnnealEngine.scan_summary, word layout in include/sga.h),
written from the definitions of the words in numpy, fp64 and Python integers -- not from the kernels.  Shared by the
tests that hold the device words against it (tests/test_set_time_scans_gpu.py), the host test of this module
(tests/test_scan_reference_host.py) and tests/batch_fx_cases.py; no test lives here.

Exponent words follow sga_classify::span_add: the binary exponents of the true highest and lowest set bit of any
non-zero value, subnormals included, zero ignored.  Row maxima are the fp32 rounding of the exact sum (math.fsum)."""
import math

import numpy as np

DENSE_WORDS = ("not_int8", "not_ternary", "row_abs_max", "not_integral", "asymmetric_or_diagonal", "exp_hi", "exp_lo",
               "j_abs_max")
CSR_WORDS = ("bad_rowptr", "bad_column", "not_integral", "unsorted", "diagonal", "asymmetric", "row_abs_max", "exp_hi",
             "exp_lo", "row_j_abs_max", "longest_row")


def f32_bits(x):
    """The bits of float32(x) as a non-negative int32 (x >= 0)."""
    return int(np.float32(x).view(np.int32))


def bit_span(values):
    """(e_hi, e_lo): exponents of the highest and the lowest set bit over the non-zero finite fp32 `values`; None if
    there is none.  From the bit pattern: exponent field 0 holds the subnormals, value = mantissa 2^-149."""
    v = np.ascontiguousarray(values, dtype=np.float32).ravel()
    v = v[(v != 0) & np.isfinite(v)]
    if v.size == 0:
        return None
    bits = v.view(np.int32) & 0x7FFFFFFF
    field = bits >> 23
    mant = (bits & 0x7FFFFF) | ((field > 0).astype(np.int32) << 23)
    unit = np.where(field > 0, field - 150, -149)  # the exponent of the mantissa's bit 0
    # bit positions inside the 24-bit mantissa: frexp of an integer below 2^24 is exact in fp32
    top = np.frexp(mant.astype(np.float32))[1] - 1
    low = np.frexp((mant & -mant).astype(np.float32))[1] - 1  # m & -m: the lowest set bit alone
    assert np.all((mant >> top) == 1) and np.all(mant & ((1 << (low + 1)) - 1) == (1 << low))
    return int((unit + top).max()), int((unit + low).min())


def exponent_words(values):
    """[1024 + e_hi, 1024 - e_lo], [0, 0] without a non-zero value."""
    s = bit_span(values)
    return [0, 0] if s is None else [1024 + s[0], 1024 - s[1]]


def max_exact_sum(terms, extra):
    """max_i (sum of the i-th row of the non-negative fp64 `terms` + extra_i), the sum exact: the rows are ranked by
    their fp64 sums (relative error at most len 2^-53) and math.fsum decides among those within 10^-9 of the best."""
    approx = terms.sum(1) + extra
    if not np.all(np.isfinite(approx)):
        return float("nan")
    best = 0.0
    for i in np.nonzero(approx >= approx.max() * (1.0 - 1e-9))[0]:
        best = max(best, math.fsum(list(terms[i]) + [extra[i]]))
    return best


def not_integral_bits(J_values, h):
    J_values, h = np.asarray(J_values, np.float32), np.asarray(h, np.float32)
    return ((0 if np.all(J_values == np.rint(J_values)) else 1) | (0 if np.all(h == np.rint(h)) else 2) |
            (0 if np.all(2 * h == np.rint(2 * h)) else 4))


def dense_words(Js, hs):
    """The eight words of a dense problem ([n, n] with [n]) or of a stacked batch ([M, n, n] with [M, n])."""
    Js = np.asarray(Js, np.float32)
    Js = Js.reshape((-1,) + Js.shape[-2:])
    J = Js.reshape(-1, Js.shape[-1])
    h = np.asarray(hs, np.float32).reshape(-1)
    assert h.size == J.shape[0]
    integer = bool(np.all(J == np.rint(J)))
    jmax = float(np.abs(J).max())
    row = max_exact_sum(np.abs(J.astype(np.float64)), np.abs(h.astype(np.float64)))
    symmetric = all(np.array_equal(Jm, Jm.T) and not np.any(np.diag(Jm)) for Jm in Js)
    return [0 if integer and jmax <= 127 else 1, 0 if integer and jmax <= 1 else 1, f32_bits(row), not_integral_bits(J, h),
            0 if symmetric else 1] + exponent_words(J) + [f32_bits(jmax)]


def scan_words(Js, hs):
    """What the set-time scans hand to classify_dense for the stacked batch (tests/batch_fx_cases.py's name for it)."""
    return dense_words(Js, hs)


def dense_as_csr(J):
    """(rowptr int32, colidx int32, val float32) of the non-zeros of each row in ascending column order; -0.0 is not an
    entry."""
    J = np.asarray(J, np.float32)
    keep = J != 0
    rowptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int32)
    rows, cols = np.nonzero(keep)  # row-major: ascending columns within a row
    return rowptr, cols.astype(np.int32), J[rows, cols].astype(np.float32)


def csr_words(rowptr, colidx, val, h):
    """The CSR words in enum order plus the longest row, and the two structure verdicts in front: a list of eleven.  With
    a bad rowptr nothing else is looked at (the list ends there: [1]); with a bad column the values are not (then [0, 1])."""
    rp = np.asarray(rowptr, np.int64)
    ci = np.asarray(colidx, np.int64)
    v = np.asarray(val, np.float32)
    h = np.asarray(h, np.float32)
    n, nnz = rp.size - 1, ci.size
    assert v.size == nnz and h.size == n
    if rp[0] != 0 or rp[n] != nnz or np.any(np.diff(rp) < 0) or np.any(rp < 0) or np.any(rp > nnz):
        return [1]
    if nnz and (ci.min() < 0 or ci.max() >= n):
        return [0, 1]
    length = np.diff(rp)
    row = np.repeat(np.arange(n, dtype=np.int64), length)
    inner = np.ones(nnz, bool)
    inner[rp[:-1][length > 0]] = False  # an entry with a left neighbour in its own row
    unsorted = bool(np.any(inner[1:] & (ci[:-1] >= ci[1:]))) if nnz > 1 else False
    diagonal = bool(np.any((ci == row) & (v != 0)))
    # J_ij as held: duplicates of one (i, j) summed (test inputs keep such sums exact); an absent entry is 0
    key, inv = np.unique(row * n + ci, return_inverse=True)
    total = np.zeros(key.size)
    np.add.at(total, inv.ravel(), v.astype(np.float64))
    mirror = (key % n) * n + key // n
    at = np.minimum(np.searchsorted(key, mirror), key.size - 1) if key.size else mirror
    other = np.where(key[at] == mirror, total[at], 0.0) if key.size else total
    asymmetric = bool(np.any((key // n != key % n) & (other != total)))
    # row sums: exact, over the stored entries
    a = np.abs(v.astype(np.float64))
    ah = np.abs(h.astype(np.float64))
    approx = np.bincount(row, weights=a, minlength=n) if nnz else np.zeros(n)

    def best(extra):
        tot = approx + extra
        out = 0.0
        for i in np.nonzero(tot >= tot.max() * (1.0 - 1e-9))[0]:
            out = max(out, math.fsum(list(a[rp[i]:rp[i + 1]]) + [extra[i]]))
        return out
    return [0, 0, not_integral_bits(v, h), int(unsorted), int(diagonal), int(asymmetric), f32_bits(best(ah))] + \
        exponent_words(v) + [f32_bits(best(np.zeros(n))), int(length.max())]
