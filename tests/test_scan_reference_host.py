"""The plain reference of the set-time scans (tests/scan_reference.py) is itself held against what is already pinned,
without a GPU: its exponent words against sga_classify::span_add (the print of tests/c_abi/classify_cases.cpp), its dense
words against the numpy restatement tests/batch_fx_cases.py carried before, its CSR row maxima against the instances of
tests/range_edges.py built to carry an exact bound, and every word against small matrices worked out by hand.  Then the
read-out's place in the C ABI, and tests/c_abi/scan_classify.cpp on hand-made words."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import batch_fx_cases as cases
import range_edges as edges
import scan_reference as ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc")


def _compile(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "c_abi", name + ".cpp"), "-o", exe, "-L", CSRC, "-lsga",
                    "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    return exe


F32_MAX = float(np.finfo(np.float32).max)
SPAN_VALUES = {  # the values tests/c_abi/classify_cases.cpp hands to span_add, by the name it prints
    "1.0": [1.0], "3.0": [3.0], "0.75": [0.75], "-0.75 and 1.0": [-0.75, 1.0],
    "0 inf nan": [0.0, -0.0, np.inf, -np.inf, np.nan], "2^-149": [2.0 ** -149], "3 x 2^-149": [3 * 2.0 ** -149],
    "largest float": [F32_MAX]}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_exponent_words_are_span_adds(tmp_path):
    out = subprocess.run([_compile(tmp_path, "classify_cases")], check=True, capture_output=True, text=True).stdout
    lines = dict(line.split(": ", 1) for line in out.split("# float bit span\n")[1].split("# ")[0].splitlines())
    for name, values in SPAN_VALUES.items():
        s = ref.bit_span(np.asarray(values, np.float32))
        assert lines[name] == ("none" if s is None else f"hi={s[0]} lo={s[1]}"), (name, s, lines[name])
        want = [0, 0] if s is None else [1024 + s[0], 1024 - s[1]]
        assert ref.exponent_words(np.asarray(values, np.float32)) == want
    # the words span_of_words reads back: 2^20 beside 2^-21 is the pinned "words 1044 1045: hi=20 lo=-21"
    assert ref.exponent_words(np.asarray([2.0 ** 20, 0.0, -2.0 ** -21], np.float32)) == [1044, 1045]
    assert lines["words 1044 1045"] == "hi=20 lo=-21"


def test_exponents_of_subnormals_and_mixed_values_by_hand():
    assert ref.bit_span(np.asarray([2.0 ** -126], np.float32)) == (-126, -126)     # the smallest normal
    assert ref.bit_span(np.asarray([2.0 ** -127], np.float32)) == (-127, -127)     # subnormal, mantissa 2^22
    assert ref.bit_span(np.asarray([3 * 2.0 ** -149, 2.0 ** -126], np.float32)) == (-126, -149)
    assert ref.bit_span(np.asarray([(2 ** 23 - 1) * 2.0 ** -149], np.float32)) == (-127, -149)  # the largest subnormal
    assert ref.bit_span(np.asarray([1.0 + 2.0 ** -23, -6.0], np.float32)) == (2, -23)
    assert ref.bit_span(np.zeros(5, np.float32)) is None


def _scan_words_before(Js, hs):
    """tests/batch_fx_cases.py's scan_words as it stood before it moved to scan_reference (frexp exponents, fp64 numpy
    sums), kept here to show that the move changed no word of its cases."""
    J = Js.reshape(-1, Js.shape[-1]).astype(np.float32)
    h = hs.reshape(-1).astype(np.float32)
    integer = bool(np.all(J == np.rint(J)))
    nz = J[J != 0].astype(np.float64)
    mant, ex = np.frexp(np.abs(nz))
    im = np.rint(np.ldexp(mant, 24)).astype(np.int64)
    low = np.zeros_like(im)
    for b in range(24):
        low += ((im & ((1 << (b + 1)) - 1)) == 0).astype(np.int64)
    hi, lo = int((ex - 1).max()), int((ex - 24 + low).min())
    row = np.float32((np.abs(J.astype(np.float64)).sum(1) + np.abs(h.astype(np.float64))).max())
    nonint = (0 if integer else 1) | (0 if np.all(h == np.rint(h)) else 2) | (0 if np.all(2 * h == np.rint(2 * h)) else 4)
    symmetric = all(np.array_equal(Jm, Jm.T) and not np.any(np.diag(Jm)) for Jm in Js)
    fits_i8 = integer and float(np.abs(J).max()) <= 127
    ternary = integer and float(np.abs(J).max()) <= 1
    return [0 if fits_i8 else 1, 0 if ternary else 1, int(row.view(np.int32)), nonint, 0 if symmetric else 1, 1024 + hi,
            1024 - lo, int(np.float32(np.abs(J).max()).view(np.int32))]


@pytest.mark.parametrize("case", ["case_a", "case_b", "case_c", "case_d", "case_e"])
def test_dense_words_of_the_batch_cases_are_unchanged(case):
    Js, hs = getattr(cases, case)()
    assert cases.scan_words is ref.scan_words
    assert ref.dense_words(Js, hs) == _scan_words_before(Js, hs)
    assert ref.dense_words(Js[1], hs[1]) == _scan_words_before(Js[1:2], hs[1:2])  # one model, handed over as [n, n]


@pytest.mark.parametrize("L", [32767, 32768, (1 << 24) - 1, 1 << 24])
def test_csr_words_of_the_saturating_instance_carry_exactly_L(L):
    csr, h, _, J = edges.saturating_csr(L)
    w = ref.csr_words(*csr, h)
    assert w[:6] == [0, 0, 0, 0, 0, 0]
    assert w[9] == ref.f32_bits(L) and np.int32(w[9]).view(np.float32) == L
    exact = np.abs(J).astype(np.int64).sum(1) + np.abs(h).astype(np.int64)  # integers: exact in int64
    assert w[6] == ref.f32_bits(int(exact.max())) and exact[0] == L + (3 << 15)
    assert w[10] == 80 == int((J != 0).sum(1).max()) and w[7:9] == ref.exponent_words(J)
    assert ref.csr_words(*ref.dense_as_csr(J), h) == w
    d = ref.dense_words(J, h)
    assert d[2] == w[6] and d[5:7] == w[7:9] and d[3] == w[2] and d[4] == 0


def test_csr_words_by_hand():
    #     0  2  0  0
    #     2  0 .5  0      h = (1, 0, -1.5, 0.25)
    #     0 .5  0 -3
    #     0  0 -3  0
    rp, ci = [0, 1, 3, 5, 6], [1, 0, 2, 1, 3, 2]
    v, h = [2, 2, .5, .5, -3, -3], [1, 0, -1.5, .25]
    base = [0, 0, 1 | 2 | 4, 0, 0, 0, ref.f32_bits(5.0), 1024 + 1, 1024 + 1, ref.f32_bits(3.5), 2]
    assert ref.csr_words(rp, ci, v, h) == base
    assert ref.csr_words(rp, ci, v, [1, 0, -1.5, 0])[2] == 1 | 2           # halves only
    assert ref.csr_words(rp, ci, [2, 2, 1, 1, -3, -3], [1, 0, -1, 0])[2] == 0
    w = ref.csr_words(rp, [1, 2, 0, 1, 3, 2], [2, .5, 2, .5, -3, -3], h)   # row 1 descending
    assert w == base[:3] + [1] + base[4:]
    w = ref.csr_words([0, 1, 4, 6, 7], [1, 0, 2, 2, 1, 3, 2], [2, 2, .25, .25, .5, -3, -3], h)  # (1, 2) twice: sums to .5
    assert w[3] == 1 and w[5] == 0 and w[10] == 3 and w[8] == 1024 + 2
    assert ref.csr_words(rp, ci, [2, 2, .5, .5, -3, 3], h)[5] == 1         # J_23 = -3, J_32 = 3
    assert ref.csr_words([0, 1, 3, 4, 5], [1, 0, 2, 3, 2], [2, 2, .5, -3, -3], h)[5] == 1  # J_21 not stored
    w = ref.csr_words([0, 2, 4, 6, 7], [0, 1, 0, 2, 1, 3, 2], [7, 2, 2, .5, .5, -3, -3], h)    # J_00 = 7
    assert w[4] == 1 and w[5] == 0 and w[6] == ref.f32_bits(10.0)
    assert ref.csr_words([0, 2, 4, 6, 7], [0, 1, 0, 2, 1, 3, 2], [0, 2, 2, .5, .5, -3, -3], h)[4] == 0  # a stored zero
    # the first entry of a row is not compared with the last of the row before; an empty row in between
    assert ref.csr_words([0, 1, 1, 2], [2, 0], [1, 1], [0, 0, 0])[3:6] == [0, 0, 0]
    # structure verdicts
    assert ref.csr_words([1, 1, 3, 5, 6], ci, v, h) == [1] and ref.csr_words([0, 1, 3, 5, 7], ci, v, h) == [1]
    assert ref.csr_words([0, 3, 1, 5, 6], ci, v, h) == [1] and ref.csr_words([0, -1, 3, 5, 6], ci, v, h) == [1]
    assert ref.csr_words(rp, [1, 0, 2, 1, 4, 2], v, h) == [0, 1] and ref.csr_words(rp, [-1, 0, 2, 1, 3, 2], v, h) == [0, 1]


def test_dense_words_by_hand_and_dense_as_csr():
    J = np.asarray([[0, 2, 0, 0], [2, 0, .5, 0], [0, .5, 0, -3], [0, 0, -3, 0]], np.float32)
    h = np.asarray([1, 0, -1.5, .25], np.float32)
    assert ref.dense_words(J, h) == [1, 1, ref.f32_bits(5.0), 7, 0, 1025, 1025, ref.f32_bits(3.0)]
    K = J.copy()
    K[3, 0] = -0.0
    rp, ci, v = ref.dense_as_csr(K)
    assert rp.tolist() == [0, 1, 3, 5, 6] and ci.tolist() == [1, 0, 2, 1, 3, 2] and v.tolist() == [2, 2, .5, .5, -3, -3]
    assert ref.dense_words(K, h)[4] == 0  # -0.0 == 0.0
    K[3, 0] = 1
    assert ref.dense_words(K, h)[4] == 1
    K[3, 0], K[3, 3] = 0, 1
    assert ref.dense_words(K, h)[4] == 1
    I = np.asarray([[0, 127], [127, 0]], np.float32)
    assert ref.dense_words(I, [0, 0])[:2] == [0, 1] and ref.dense_words(I + I.T / 127, [0, 0])[:2] == [1, 1]
    assert ref.dense_words(I / 127, [0, 0])[:2] == [0, 0] and ref.dense_words(0 * I, [0, 0])[5:7] == [0, 0]
    # a batch is scanned stacked: model 1's defect shows in the one set of words
    assert ref.dense_words(np.stack([J, K]), np.stack([h, h]))[4] == 1
    # the exact sum: 2^24 + 1 is no fp32 number and a tie: to even, 2^24; with one more 1 it rounds up to 2^24 + 2
    big = np.zeros((4, 4), np.float32)
    big[0, 1], big[0, 2] = 2.0 ** 24, 1.0
    assert ref.dense_words(big, np.zeros(4))[2] == ref.f32_bits(2.0 ** 24)
    assert ref.dense_words(big, [1, 0, 0, 0])[2] == ref.f32_bits(2.0 ** 24 + 2)


def test_read_out_is_bound_and_versioned():
    import spin_glass_anneal_rl_amd as sg
    N = sg._native
    assert N.lib().sga_version() >= 1500
    assert "sga_get_scan_summary" in [s[0] for s in N.SYMBOLS] and hasattr(sg.AnnealEngine, "scan_summary")
    rc = N.lib().sga_get_scan_summary(None, 0, None, None, 0, None)
    assert rc == N.ERR_INVALID and "NULL" in N.last_error()
    header = open(os.path.join(ROOT, "include", "sga.h")).read()
    assert len(ref.DENSE_WORDS) == 8 and len(ref.CSR_WORDS) == 11 and "11 words per model" in header and "8 words" in header
    kernels = open(os.path.join(CSRC, "sga_kernels.h")).read()
    assert "CSR_FLAG_COUNT = 10" in kernels and "int[CSR_FLAG_COUNT] = int[10]" in kernels


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_scan_classify_reads_words_as_the_setters_do(tmp_path):
    exe = _compile(tmp_path, "scan_classify")
    b = ref.f32_bits
    args = (["dense", 64, 1, 0, 0, b(63.0), 0, 0, 1024, 1024, b(1.0)] +                       # +-1, integer h
            ["dense", 64, 1, 1, 1, b(40000.0), 2, 0, 1034, 1024, b(1000.0)] +                 # integers, half-integer h
            ["dense", 64, 3, 1, 1, b(10.0), 1, 1, 1024, 1034, b(1.0)] +                       # grid 2^-10, asymmetric
            ["csr", 64, 0, 0, 0, 0, 0, 0, b(16777215.0), 1024, 1024, b(32767.0), 8] +         # classify_cases: "16777215"
            ["csr", 64, 0, 0, 0, 0, 0, 0, b(16777216.0), 1024, 1024, b(16777216.0), 8] +      # ... "16777216"
            ["ragged", 2, 64, 0, 0, 0, 0, 0, 0, b(10.0), 1024, 1024, b(10.0), 8,
             32, 0, 0, 2, 1, 0, 0, b(20.5), 1024, 1024, b(20.0), 8])
    out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out == ["dense storage=2 acc=0 table_m=63 clf=1 bits=16 scale=1 dE=1",
                   "dense storage=1 acc=0 table_m=0 clf=1 bits=32 scale=2 dE=1",
                   "dense storage=1 acc=1 table_m=0 clf=0 bits=16 scale=1 dE=0",
                   "csr acc=0 table_m=2048 scale=1 clf=1 dE=1 sorted=1",
                   "csr acc=2 table_m=0 scale=1 clf=0 dE=1 sorted=1",
                   "ragged acc=0 table_m=41 scale=2 sorted=0"], out
