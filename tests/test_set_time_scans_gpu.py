"""The set-time scans of csrc/sga_misc.hip against the plain reference tests/scan_reference.py, element by element.

Every sweep form is chosen from the few words these scans write.  Here AnnealEngine.scan_summary() -- the words as the
setter read them back -- is held against the reference word for word, over base problems of every value class with ONE
planted element at the places a scan can lose: tile and wave boundaries, the last row and column, rows and flat indices
beyond a grid-stride cap, the last model of a batch, the column next to row padding.  describe() and route_query() must
carry the class sga_classify gives for those words (tests/c_abi/scan_classify.cpp, host code).  One chain per kind of
plant then walks two sweeps against the oracle bit for bit: what fails if a word is wrong in a way the read-out shares.
Structure defects and non-finite values are refused.  Everything is exact equality; the one derived condition (Gaussian
row sums away from fp32 rounding ties) is asserted on the inputs.
"""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import scan_reference as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

INF = float("inf")
BASES = ["pm1", "i127", "i30000", "grid", "gauss"]


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


@pytest.fixture(scope="module")
def eng(sg):
    """One engine for the module: every case sets a new problem on it (as a long-lived caller does)."""
    with sg.AnnealEngine(0) as e:
        yield e


@pytest.fixture(scope="module")
def classify(tmp_path_factory):
    """words -> the class sga_classify gives them: tests/c_abi/scan_classify.cpp, one run for a list of cases."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    csrc = os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("scan_classify") / "scan_classify")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "c_abi", "scan_classify.cpp"), "-o", exe, "-L", csrc, "-lsga",
                    "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)

    def run(cases):
        args = [str(a) for c in cases for a in c]
        out = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [dict((k, int(v)) for k, v in (f.split("=") for f in line.split()[1:])) for line in out]
    return run


# ----------------------------------------------------------------------------- base problems and plants
def sym(A):
    U = np.triu(A, 1)
    return (U + U.T).astype(np.float32)


def tie_distance(total):
    """|total - nearest fp32 rounding tie| / total, of an exact fp64 value inside the normal fp32 range."""
    m, ex = math.frexp(total)            # total = m 2^ex, m in [0.5, 1): fp32 spacing 2^(ex - 24)
    t = math.ldexp(m, 25)                # in half-spacings: ties are the odd integers
    k = math.floor(t)
    tie = k if k % 2 else k + 1
    return abs(t - tie) / t


def fp64_sum_is_exact(terms):
    """Every partial sum of these fp32 magnitudes, in any order, is an fp64 number: all set bits lie within 53 places once
    the carries of len(terms) additions are counted.  Then the device's sum IS the exact sum and a tie rounds one way."""
    span = ref.bit_span(np.asarray(terms, np.float32))
    return span is None or span[0] - span[1] + 1 + max(len(terms) - 1, 1).bit_length() <= 53


def rows_clear_of_ties(approx, terms):
    """The derived condition of the module: every row whose exact sum lies within two fp32 ulps of the maximum is farther
    than 2^-40 relative from a rounding tie -- the device's fp64 sum (its own order, n 2^-53 relative) then rounds to
    the reference's fp32 value -- unless the row is so short and narrow that its fp64 sum is exact in any order (a
    handful of CSR entries: such a sum often IS a tie, and rounds to even on the device as in the reference).
    approx: the rows' fp64 sums (they pick the rows worth an exact sum); terms(i): row i's magnitudes."""
    top = float(approx.max())
    if top == 0.0:
        return True
    ulp = math.ldexp(1.0, math.frexp(top)[1] - 24)
    rows = [terms(i) for i in np.nonzero(approx >= top - 3 * ulp)[0]]
    tot = [math.fsum(t) for t in rows]
    return all(tie_distance(x) > 2.0 ** -40 or fp64_sum_is_exact(t) for x, t in zip(tot, rows) if x >= max(tot) - 2 * ulp)


def gauss_rows_clear_of_ties(J, h):
    J, h = J.reshape(-1, J.shape[-1]), h.reshape(-1)
    a, ah = np.abs(J.astype(np.float64)), np.abs(h.astype(np.float64))
    return rows_clear_of_ties(a.sum(1) + ah, lambda i: list(a[i]) + [ah[i]])


def csr_rows_clear_of_ties(rp, v, h):
    """... for both CSR maxima: max_i sum_j |J_ij| with and without |h_i|."""
    rp = np.asarray(rp, np.int64)
    a, ah = np.abs(np.asarray(v, np.float64)), np.abs(np.asarray(h, np.float64))
    approx = np.bincount(np.repeat(np.arange(len(h)), np.diff(rp)), weights=a, minlength=len(h))
    return all(rows_clear_of_ties(approx + x, lambda i: list(a[rp[i]:rp[i + 1]]) + [x[i]]) for x in (ah, 0 * ah))


_bases = {}


def base(name, n, seed=0):
    """(J [n, n] symmetric with zero diagonal, h [n] integer) of one value class; cached, never modified."""
    key = (name, n, seed)
    if key not in _bases:
        rng = np.random.RandomState(1000 * seed + n + 7 * BASES.index(name))
        if name == "pm1":
            J = sym(rng.randint(0, 2, (n, n)) * 2.0 - 1.0)
        elif name == "i127":
            J = sym(rng.randint(-126, 127, (n, n)).astype(np.float64))
            J[2, 7] = J[7, 2] = 127.0
        elif name == "i30000":
            J = sym(rng.randint(-30000, 30001, (n, n)).astype(np.float64))
            J[2, 7] = J[7, 2] = -30000.0
        elif name == "grid":
            J = sym(np.rint(rng.randn(n, n) * 1024.0) / 1024.0)
        else:
            for attempt in range(50):  # the seed is chosen on the CPU: row sums clear of rounding ties
                J = sym(np.random.RandomState(1000 * seed + n + 100 * attempt).randn(n, n))
                if gauss_rows_clear_of_ties(J, np.zeros(n)):
                    break
        h = rng.randint(-3, 4, n).astype(np.float32)
        if name == "gauss":
            h[:] = 0.0  # (the tie condition above was checked with these fields)
        J.setflags(write=False), h.setflags(write=False)
        _bases[key] = (J, h)
    return _bases[key]


def span_value(J, terms, total):
    """A value whose lowest set bit brings span + carries of J (sga_classify::fp64_exact_any_order: highest - lowest set
    bit + 1 + carry_bits(terms)) to `total`, if J's own lowest bit lies above it: 52 is a single bit, 53 that bit and
    the one below (one extra low bit)."""
    hi = ref.bit_span(J)[0]
    carry = 0
    while (1 << carry) < max(terms, 1):
        carry += 1
    top = hi - 51 + carry
    return np.float32(2.0 ** top if total == 52 else 1.5 * 2.0 ** top)


DENSE_KINDS = ["half", "128", "2", "asym", "asym_T", "diag", "span52", "span53", "h_half", "h_quarter", "row24_edge", "row24",
               "row15_edge", "row15"]
# on the +-1 base each kind changes this word against its own base (row kinds: against their edge matrix)
FLIPS = {"half": 3, "128": 0, "2": 1, "asym": 4, "asym_T": 4, "diag": 4, "span53": 6, "h_half": 3, "h_quarter": 3, "row24": 2,
         "row15": 2}


def plant(J, h, kind, r, c, terms, clear=True):
    """A copy of (J, h) with one element planted at (r, c), mirrored where the plant is not itself the asymmetry.  Row
    kinds: row r is brought to sum_j |J_rj| + |h_r| = 2^24 - 1 | 32767 exactly (`_edge`: one large coupling to a filler
    site, no field on either; dense: rows r and the filler's cleared first) and the plant lifts |J_rc| by one.  Returns None where
    the construction does not exist (the rest of the row already exceeds the target)."""
    J, h = J.copy(), h.copy()
    if kind in ("half", "128", "2"):
        J[r, c] = J[c, r] = {"half": 0.5, "128": 128.0, "2": 2.0}[kind]
    elif kind == "asym":
        J[r, c] += 1.0
    elif kind == "asym_T":
        J[c, r] += 1.0
    elif kind == "diag":
        J[r, r] = 1.0
    elif kind in ("span52", "span53"):
        J[r, c] = J[c, r] = span_value(J, terms, int(kind[4:]))
    elif kind == "h_half":
        h[r] = 0.5
    elif kind == "h_quarter":
        h[c] = 0.25
    else:
        target = (1 << 24) if kind.startswith("row24") else (1 << 15)
        nz = np.nonzero(J[r])[0]
        f = int([j for j in nz if j not in (r, c)][len(nz) // 2])  # an existing entry of row r: the filler
        if clear:
            J[r, :] = J[:, r] = 0.0
            J[f, :] = J[:, f] = 0.0
        J[r, c] = J[c, r] = 1.0
        h[r] = h[f] = 0.0  # (the filler's row holds the large coupling too: below row r's sum without a field)
        J[r, f] = J[f, r] = 0.0
        rest = float(np.abs(J[r].astype(np.float64)).sum())
        big = target - 1 - rest
        if big != np.rint(big) or big < 1:
            return None
        J[r, f] = J[f, r] = -big
        if not kind.endswith("_edge"):
            J[r, c] = J[c, r] = 2.0
    return J, h


def dense_positions(n):
    pos = [(0, 1), (0, n - 1), (n - 2, n - 1), (63, 64), (63, 127), (64, 128), (65, 66)]
    return pos + [(n - 1, 64 * k) for k in range((n - 1) // 64 + 1) if 64 * k != n - 1]


LARGE_POSITIONS = [(954, 500), (1099, 1024), (960, 255), (1000, 1099)]  # flat index r n + c > 4096 * 256

STORAGE = {1: "f32", 2: "i8", 3: "t2"}


def dense_class_matches(e, want):
    q, d = e.route_query(), e.describe()
    got = dict(storage=q.storage, acc=q.acc, table_m=q.table_m, clf=q.clf_ok, bits=q.clf_bits, scale=q.clf_scale)
    name = "i32" if want["storage"] != 1 else ("f32", "f64-exact", "f64-canonical")[want["acc"]]
    ok = all(got[k] == want[k] for k in got) and q.kind == 0 and \
        f" storage={STORAGE[want['storage']]} acc={name} " in d and f" table_m={want['table_m']} " in d
    return ok, (got, d)


def csr_path(c):
    if c["acc"] == 0 and c["table_m"] > 0:
        return "half-integer-fast" if c["scale"] == 2 else "integer-fast"
    return ("general acc=f32-exact", "general acc=f32-exact", "general acc=f64-exact", "general acc=f64-canonical")[c["acc"]]


class Checker:
    """Sets problems, compares the words with the reference at once, and the classes at the end in one classifier run."""

    def __init__(self, e, classify, ties=False):
        self.e, self.classify, self.pending = e, classify, []
        self.ties = ties  # Gaussian couplings: assert the inputs' row sums clear of fp32 rounding ties

    def dense(self, J, h, tag, setter=None):
        e = self.e
        assert not self.ties or gauss_rows_clear_of_ties(J, h), tag
        (setter or (lambda: e.set_dense_batch(J, h) if J.ndim == 3 else e.set_dense(J, h)))()
        kind, words = e.scan_summary()
        want = ref.dense_words(J, h)
        assert kind == 0 and words == want, (tag, dict(zip(ref.DENSE_WORDS, zip(words, want))))
        n, M = J.shape[-1], (J.shape[0] if J.ndim == 3 else 1)
        q, d = e.route_query(), e.describe()
        self.pending.append((["dense", n, M] + words, "dense", (q.kind, q.storage, q.acc, q.table_m, q.clf_ok, q.clf_bits,
                                                               q.clf_scale), d, tag))
        return words

    def csr(self, rp, ci, v, h, tag, wide=False):
        e = self.e
        assert not self.ties or csr_rows_clear_of_ties(rp, v, h), tag
        e.set_csr(np.asarray(rp, np.int64 if wide else np.int32), ci, v, h)
        kind, words = e.scan_summary()
        want = ref.csr_words(rp, ci, v, h)
        assert kind == 1 and words == want, (tag, dict(zip(ref.CSR_WORDS, zip(words, want))))
        q, d = e.route_query(), e.describe()
        assert q.nnz == len(ci) and q.max_row_len == want[10], tag
        self.pending.append((["csr", len(h)] + words, "csr", (q.kind, q.acc, q.table_m, q.table_scale, q.clf_ok), d, tag))
        return words

    def ragged(self, problems, tag):
        e = self.e
        e.set_csr_batch(problems)
        args = ["ragged", len(problems)]
        for m, p in enumerate(problems):
            assert not self.ties or csr_rows_clear_of_ties(p[0], p[2], p[3]), (tag, m)
            kind, words = e.scan_summary(m)
            want = ref.csr_words(*p)
            assert kind == 1 and words == want, (tag, m, dict(zip(ref.CSR_WORDS, zip(words, want))))
            args += [len(p[3])] + words
        q, d = e.route_query(), e.describe()
        self.pending.append((args, "ragged", (q.kind, q.acc, q.table_m, q.table_scale), d, tag))

    def finish(self):
        classes = self.classify([p[0] for p in self.pending])
        for c, (_, what, got, d, tag) in zip(classes, self.pending):
            if what == "dense":
                name = "i32" if c["storage"] != 1 else ("f32", "f64-exact", "f64-canonical")[c["acc"]]
                assert got == (0, c["storage"], c["acc"], c["table_m"], c["clf"], c["bits"], c["scale"]), (tag, got, c)
                assert f" storage={STORAGE[c['storage']]} acc={name} " in d and f" table_m={c['table_m']} " in d, (tag, d, c)
            elif what == "csr":
                assert got == (1, c["acc"], c["table_m"], c["scale"], c["clf"]), (tag, got, c)
                assert f" path={csr_path(c)} table_m={c['table_m']} " in d, (tag, d, c)
            else:
                assert got == (1, c["acc"], c["table_m"], c["scale"]), (tag, got, c)
                assert f" path={csr_path(c)} table_m={c['table_m']} " in d, (tag, d, c)
        self.pending = []
        return classes


def run_dense_plants(chk, J0, h0, positions, name, lift=lambda J, h: (J, h)):
    """Every kind at every position; `lift` places the planted model into what is handed over (a batch)."""
    n = J0.shape[0]
    base_words = chk.dense(*lift(J0, h0), (name, "base"))
    for r, c in positions:
        edge = {}
        for kind in DENSE_KINDS:
            p = plant(J0, h0, kind, r, c, n)
            if p is None:
                assert name != "pm1", (kind, r, c)
                continue
            w = chk.dense(*lift(*p), (name, kind, r, c))
            if kind.endswith("_edge"):
                edge[kind[:5]] = w
            if name == "pm1" and kind in FLIPS:
                before = edge[kind] if kind in edge else base_words
                assert w[FLIPS[kind]] != before[FLIPS[kind]], (kind, r, c, w, before)
    return chk.finish()


# ----------------------------------------------------------------------------- dense
@pytest.mark.parametrize("name", BASES)
def test_dense_n193_every_plant_at_every_tile_edge(eng, classify, name):
    """n = 193: three whole 64-tiles and a one-wide partial tile in check_symmetric_kernel; one pass of the row kernel."""
    J, h = base(name, 193)
    run_dense_plants(Checker(eng, classify, name == "gauss"), J, h, dense_positions(193), name)


@pytest.mark.parametrize("name", BASES)
def test_dense_n1100_plants_beyond_the_grid_stride(eng, classify, name):
    """n = 1100: n^2 > 4096 * 256, so scan_values_kernel grid-strides and rows >= 954 lie in its second pass; the columns
    wrap the 256 threads of dense_row_abs_max_kernel four times (columns 255 | 256, 1024, 1099)."""
    J, h = base(name, 1100)
    assert all(r * 1100 + c > 4096 * 256 for r, c in LARGE_POSITIONS)
    run_dense_plants(Checker(eng, classify, name == "gauss"), J, h, LARGE_POSITIONS, name)


@pytest.mark.parametrize("name", BASES)
def test_dense_batch_plants_in_model_2_only(eng, classify, name):
    """M = 3 stacked models: the plant sits in model 2's J or in model 2's h (blockIdx.z of the symmetry check, the
    stacked-row h index of the row kernel); models 0 and 1 are other draws of the same class."""
    n = 193
    others = [base(name, n, seed=s) for s in (1, 2)]

    def lift(J, h):
        return np.stack([others[0][0], others[1][0], J]), np.stack([others[0][1], others[1][1], h])
    J, h = base(name, n)
    run_dense_plants(Checker(eng, classify, name == "gauss"), J, h, [(0, n - 1), (63, 64), (n - 1, 128)], name, lift)


def test_span_plant_moves_the_class_from_f64_exact_to_canonical(eng, classify):
    """+-1 couplings: one value whose lowest bit takes span + carries to 52 keeps fp64 sums exact in any order; one
    extra low bit (53) needs the canonical order.  The class follows the words."""
    for n, (r, c) in ((193, (192, 128)), (1100, (1099, 1024))):
        J, h = base("pm1", n)
        chk = Checker(eng, classify)
        chk.dense(*plant(J, h, "span52", r, c, n), (n, 52))
        chk.dense(*plant(J, h, "span53", r, c, n), (n, 53))
        assert [k["acc"] for k in chk.finish()] == [1, 2]


def test_subnormal_couplings_report_their_true_top_bit(eng, classify):
    """Largest |J| = 3 x 2^-149 beside one of 2^-126: e_hi = -148 | -126 (sga_classify::span_add), not the exponent
    field's -127, dense and CSR alike."""
    n = 193
    for top, hi in ((3 * 2.0 ** -149, -148), (2.0 ** -126, -126)):
        J = np.zeros((n, n), np.float32)
        J[0, n - 1] = J[n - 1, 0] = np.float32(top)
        J[63, 64] = J[64, 63] = np.float32(2.0 ** -149)
        h = np.zeros(n, np.float32)
        chk = Checker(eng, classify)
        w = chk.dense(J, h, top)
        assert w[5:7] == [1024 + hi, 1024 + 149]
        w = chk.csr(*ref.dense_as_csr(J), h, top)
        assert w[7:9] == [1024 + hi, 1024 + 149]
        chk.finish()


@pytest.mark.parametrize("name", BASES)
def test_row_stride_padding_is_never_read(sg, eng, classify, name):
    """The same matrices as a strided device view (canvas[:n, :n]) and from host memory with ldJ = n + 3 through the C
    ABI; the columns [n, ldJ) hold NaN, 0.5 and asymmetric garbage.  Same words as the contiguous matrix, no refusal."""
    import torch
    n = 193
    J0, h0 = base(name, n)
    chk = Checker(eng, classify, name == "gauss")
    for case in [(J0, h0)] + [plant(J0, h0, k, n - 2, n - 1, n) for k in ("half", "asym", "128")]:
        J, h = case
        canvas = np.empty((n + 2, n + 3), np.float32)
        canvas[:, n] = np.nan
        canvas[:, n + 1] = 0.5
        canvas[:, n + 2] = np.arange(n + 2) * 1000.0 + 0.25
        canvas[n:, :] = np.inf
        canvas[:n, :n] = J
        plain = chk.dense(J, h, (name, "contiguous"))
        dev = torch.from_numpy(canvas).cuda()
        assert chk.dense(J, h, (name, "device view"), lambda: eng.set_dense(dev[:n, :n], torch.from_numpy(h.copy()).cuda())) == plain
        hh = np.ascontiguousarray(h, np.float32)

        def host():
            sg._native.check(eng._lib.sga_set_dense(eng._h, canvas.ctypes.data_as(C.c_void_p), n + 3,
                                                    hh.ctypes.data_as(C.c_void_p), n, 0), "sga_set_dense")
        assert chk.dense(J, h, (name, "host, ldJ = n + 3"), host) == plain
    chk.finish()


def test_dense_batch_with_row_stride_from_host(sg, eng, classify):
    """sga_set_dense_batch with ldJ = n + 3: model 2's rows start at 2 n ldJ; the plant in its last row and column."""
    n, M = 193, 3
    Js = np.stack([base("i127", n, seed=s)[0] for s in range(M)])
    hs = np.stack([base("i127", n, seed=s)[1] for s in range(M)])
    chk = Checker(eng, classify)
    for kind in ("half", "asym_T", "diag"):
        J2, h2 = plant(Js[2], hs[2], kind, n - 1, 128, n)
        J, h = np.stack([Js[0], Js[1], J2]), np.stack([hs[0], hs[1], h2])
        canvas = np.full((M * n, n + 3), np.nan, np.float32)
        canvas[:, :n] = J.reshape(M * n, n)
        hh = np.ascontiguousarray(h, np.float32)

        def host():
            sg._native.check(eng._lib.sga_set_dense_batch(eng._h, canvas.ctypes.data_as(C.c_void_p), n + 3,
                                                          hh.ctypes.data_as(C.c_void_p), n, M, 0), "sga_set_dense_batch")
        chk.dense(J, h, kind, host)
        with pytest.raises(sg.AnnealingError, match="model must be 0"):
            eng.scan_summary(2)
    chk.finish()


# ----------------------------------------------------------------------------- CSR
SPECIAL = {"deg64": 0, "deg1": 5, "deg63": 10, "deg200": 50, "empty": 100, "after_empty": 101, "deg65": 332}


def csr_structure(n=333):
    """A symmetric pattern with rows of 0, 1, 63, 64, 65 and 200 entries (SPECIAL) among rows of a few: the special rows
    connect to ordinary ones only, so every degree is exact."""
    rng = np.random.RandomState(5)
    A = np.zeros((n, n), bool)
    special = set(SPECIAL.values()) - {SPECIAL["after_empty"]}  # (the row after the empty one is an ordinary row)
    ordinary = np.asarray([i for i in range(n) if i not in special])
    for _ in range(3 * n):
        i, j = rng.choice(ordinary, 2, replace=False)
        A[i, j] = A[j, i] = True
    for name, r in SPECIAL.items():
        if name == "after_empty":
            continue
        want = 0 if name == "empty" else int(name[3:])
        A[r, :] = A[:, r] = False
        cols = rng.choice(ordinary, want, replace=False)
        A[r, cols] = A[cols, r] = True
    A[SPECIAL["after_empty"], SPECIAL["empty"]] = A[SPECIAL["empty"], SPECIAL["after_empty"]] = False
    deg = A.sum(1)
    assert [int(deg[SPECIAL[k]]) for k in ("empty", "deg1", "deg63", "deg64", "deg65", "deg200")] == [0, 1, 63, 64, 65, 200]
    assert deg.max() == 200 and deg[SPECIAL["after_empty"]] > 0 and not A.diagonal().any()
    return A


_csr_bases = {}


def csr_base(name, n=333):
    """Dense [n, n] holding the sparse base (zero where nothing is stored; no stored value is zero) and h."""
    if name not in _csr_bases:
        A = csr_structure(n)
        J, h = base(name, n, seed=3)
        J = J.copy()
        J[J == 0] = 1.0
        J = (J * A).astype(np.float32)
        assert np.array_equal(J != 0, A) and np.array_equal(J, J.T)
        if name == "gauss":
            assert gauss_rows_clear_of_ties(J, h)
        J.setflags(write=False)
        _csr_bases[name] = (J, h)
    return _csr_bases[name]


def csr_positions(J):
    """(row, column of its k-th entry): entries 0, 63, 64 and the last of the 200-entry row; 0 and 63 (last) of row 0;
    64 (last) of row n - 1; entry 0 of the row right after the empty row."""
    out = []
    for row, ks in ((SPECIAL["deg200"], (0, 63, 64, 199)), (SPECIAL["deg64"], (0, 63)), (SPECIAL["deg65"], (64,)),
                    (SPECIAL["after_empty"], (0,))):
        cols = np.nonzero(J[row])[0]
        out += [(row, int(cols[k])) for k in ks]
    return out


@pytest.mark.parametrize("name", BASES)
def test_csr_n333_every_plant_at_every_lane_boundary(eng, classify, name):
    J0, h0 = csr_base(name)
    chk = Checker(eng, classify, name == "gauss")
    base_words = chk.csr(*ref.dense_as_csr(J0), h0, (name, "base"))
    assert base_words[10] == 200
    for i, (r, c) in enumerate(csr_positions(J0)):
        edge = {}
        for kind in DENSE_KINDS:
            p = plant(J0, h0, kind, r, c, 200, clear=False)
            if p is None:
                assert name != "pm1" or r != SPECIAL["deg200"], (kind, r, c)
                continue
            w = chk.csr(*ref.dense_as_csr(p[0]), p[1], (name, kind, r, c), wide=bool(i & 1))
            if kind.endswith("_edge"):
                edge[kind[:5]] = w
            if name == "pm1" and r == SPECIAL["deg200"] and kind in FLIPS:
                idx = {0: 6, 1: 9, 2: 6, 3: 2, 4: 4 if kind == "diag" else 5, 6: 8}[FLIPS[kind]]
                before = edge[kind] if kind in edge else base_words
                assert w[idx] != before[idx], (kind, r, c, w, before)
    chk.finish()


def csr_insert(rp, ci, v, row, at, col, value):
    """A copy with one more stored entry in `row`, in front of its entry `at` (at = row length: behind the last)."""
    rp = np.asarray(rp).copy()
    k = int(rp[row]) + at
    rp[row + 1:] += 1
    return rp, np.insert(ci, k, col).astype(np.int32), np.insert(v, k, value).astype(np.float32)


@pytest.mark.parametrize("name", ["pm1", "grid"])
def test_csr_sortedness_across_the_lane_boundary_and_at_the_very_end(eng, classify, name):
    """A swapped pair and a duplicate column at entries 63 | 64 of the 200-entry row (two lanes of different passes of
    one wave) and at the end of the last row; the asymmetric entry in a sorted and in an unsorted matrix (both
    csr_symmetry_kernel variants)."""
    J0, h0 = csr_base(name)
    rp, ci, v = ref.dense_as_csr(J0)
    n = len(h0)
    chk = Checker(eng, classify)
    for row, a in ((SPECIAL["deg200"], 63), (n - 1, 63)):
        k = int(rp[row]) + a
        assert row != n - 1 or k + 2 == len(ci)  # the pair (63, 64) of the last row ends the arrays
        c2, v2 = ci.copy(), v.copy()
        c2[[k, k + 1]], v2[[k, k + 1]] = ci[[k + 1, k]], v[[k + 1, k]]
        w = chk.csr(rp, c2, v2, h0, (name, "swapped", row), wide=row == n - 1)
        assert w[3] == 1 and w[5] == 0
        c2 = ci.copy()
        c2[k] = ci[k + 1]  # column twice (values summed), the other column gone
        w = chk.csr(rp, c2, v, h0, (name, "duplicate, other column lost", row))
        assert w[3] == 1 and w[5] == 1
        w = chk.csr(*csr_insert(rp, ci, v, row, a + 1, int(ci[k]), 0.0), h0, (name, "duplicate with a stored zero", row))
        assert w[3] == 1 and w[5] == 0
        w = chk.csr(*csr_insert(rp, ci, v, row, a + 2, int(ci[k + 1]), 0.0), h0, (name, "duplicate behind the row", row))
        assert w[3] == 1 and w[5] == 0
    # asymmetric entry: sorted matrix (binary search), then with a swapped pair elsewhere (linear scans)
    r, c = csr_positions(J0)[2]
    Ja = J0.copy()
    Ja[r, c] += 1.0
    ra, ca, va = ref.dense_as_csr(Ja)
    assert chk.csr(ra, ca, va, h0, (name, "asymmetric, sorted"))[3:6] == [0, 0, 1]
    k = int(ra[SPECIAL["deg63"]])
    ca[[k, k + 1]], va[[k, k + 1]] = ca[[k + 1, k]].copy(), va[[k + 1, k]].copy()
    assert chk.csr(ra, ca, va, h0, (name, "asymmetric, unsorted"))[3:6] == [1, 0, 1]
    # ... and a symmetric unsorted matrix whose only difference from it is that entry
    ra, ca, va = ref.dense_as_csr(J0)
    ca[[k, k + 1]], va[[k, k + 1]] = ca[[k + 1, k]].copy(), va[[k + 1, k]].copy()
    assert chk.csr(ra, ca, va, h0, (name, "symmetric, unsorted"))[3:6] == [1, 0, 0]
    chk.finish()


def ring(name, n, seed=0):
    """Degree 4: neighbours i +- 1, i +- 2 on a ring, columns ascending; values of the base's class, no zero stored."""
    rng = np.random.RandomState(50 + seed + n)
    draw = {"pm1": lambda k: rng.randint(0, 2, k) * 2.0 - 1.0,
            "i127": lambda k: rng.randint(1, 128, k) * (rng.randint(0, 2, k) * 2.0 - 1.0),
            "i30000": lambda k: rng.randint(1, 30001, k) * (rng.randint(0, 2, k) * 2.0 - 1.0),
            "grid": lambda k: np.rint(rng.randn(k) * 1024.0) / 1024.0,
            "gauss": lambda k: rng.randn(k) + 1e-3}[name]
    w = [draw(n).astype(np.float32), draw(n).astype(np.float32)]  # w[d - 1][i]: the coupling of i and i + d
    w[0][w[0] == 0], w[1][w[1] == 0] = 1.0, 1.0
    i = np.arange(n)
    cols = np.stack([(i - 2) % n, (i - 1) % n, (i + 1) % n, (i + 2) % n], 1)
    vals = np.stack([w[1][(i - 2) % n], w[0][(i - 1) % n], w[0][i], w[1][i]], 1)
    order = np.argsort(cols, 1)
    ci = np.take_along_axis(cols, order, 1).reshape(-1).astype(np.int32)
    v = np.take_along_axis(vals, order, 1).reshape(-1).astype(np.float32)
    h = rng.randint(-3, 4, n).astype(np.float32)
    return (4 * np.arange(n + 1)).astype(np.int32), ci, v, h


def entry_of(rp, ci, i, j):
    k = int(rp[i]) + int(np.nonzero(ci[rp[i]:rp[i + 1]] == j)[0][0])
    return k


def plant_csr(prob, kind, row, at):
    """One element planted into entry `at` of `row` of a CSR problem (mirrored where it is not the asymmetry)."""
    rp, ci, v, h = (a.copy() for a in prob)
    k = int(rp[row]) + at
    col = int(ci[k])
    if kind in ("half", "128", "2"):
        v[k] = v[entry_of(rp, ci, col, row)] = {"half": 0.5, "128": 128.0, "2": 2.0}[kind]
    elif kind == "asym":
        v[k] += 1.0
    elif kind == "diag":
        rp, ci, v = csr_insert(rp, ci, v, row, int(np.searchsorted(ci[rp[row]:rp[row + 1]], row)), row, 1.0)
    elif kind == "h_half":
        h[row] = 0.5
    elif kind == "h_quarter":
        h[row] = 0.25
    elif kind == "row15":  # this row's sum_j |J_ij| to 32768 exactly (integer bases), h_i = 0
        others = float(np.abs(v[rp[row]:rp[row + 1]].astype(np.float64)).sum()) - abs(float(v[k]))
        if others != np.rint(others) or others > 30000:
            return None
        v[k] = v[entry_of(rp, ci, col, row)] = 32768.0 - others
        h[row] = 0.0
    return rp, ci, v, h


@pytest.mark.parametrize("name", BASES)
def test_csr_n33000_rows_beyond_the_block_cap(eng, classify, name):
    """33 000 rows of degree 4: the scans launch 8192 blocks x 4 waves, so rows >= 32 768 are a wave's second row."""
    n = 33000
    prob = ring(name, n)
    chk = Checker(eng, classify, name == "gauss")
    chk.csr(*prob, (name, "base"))
    cases = [("half", 32768, 0), ("asym", 32768 + 101, 3), ("128", n - 1, 3), ("diag", n - 1, 0), ("h_half", n - 1, 0),
             ("h_quarter", 32768, 0), ("2", 0, 0), ("asym", 0, 3), ("row15", 32999, 3), ("diag", 32768 + 64, 0)]
    for i, (kind, row, at) in enumerate(cases):
        p = plant_csr(prob, kind, row, at)
        if p is not None:
            chk.csr(*p, (name, kind, row, at), wide=bool(i & 1))
    chk.finish()


@pytest.mark.parametrize("name", BASES)
def test_ragged_batch_plants_in_the_last_model(sg, eng, classify, name):
    """Three models of different n; the plant in the last one, whose rows and entries lie behind the others'.  An
    asymmetric entry or a diagonal one there is refused (ragged batches need a consistent dE)."""
    J1, h1 = csr_base(name)
    first, middle, last = ring(name, 70, seed=1), ref.dense_as_csr(J1) + (h1,), ring(name, 45, seed=2)
    chk = Checker(eng, classify, name == "gauss")
    chk.ragged([first, middle, last], (name, "base"))
    for kind, row, at in (("half", 44, 3), ("128", 0, 0), ("2", 44, 0), ("h_half", 44, 0), ("h_quarter", 0, 0), ("row15", 44, 3)):
        p = plant_csr(last, kind, row, at)
        if p is not None:
            chk.ragged([first, middle, p], (name, kind, row, at))
    chk.finish()
    for kind, word in (("asym", "asymmetric J"), ("diag", "non-zero diagonal")):
        with pytest.raises(sg.AnnealingError, match="model 2: " + word):
            eng.set_csr_batch([first, middle, plant_csr(last, kind, 44, 3)])
    with pytest.raises(sg.AnnealingError, match="model index out of range"):
        eng.set_csr_batch([first, middle, last])
        eng.scan_summary(3)


def test_dense_matrix_kept_as_csr_reports_the_csr_words(eng, classify):
    """A sparse integer matrix handed over dense under field cache OFF is kept as CSR (from_dense = 1): non-zeros at
    columns 0, 63, 64, 127, 128 and n - 1 (dense_row_nnz_kernel / dense_to_csr_kernel walk a row in 64-column steps),
    a -0.0 and an empty row.  Words, nnz and the longest row are those of the reference's own conversion."""
    n = 4097
    rng = np.random.RandomState(9)
    J = np.zeros((n, n), np.float32)
    i, j = rng.randint(0, n, 3 * n), rng.randint(0, n, 3 * n)
    keep = i != j
    J[i[keep], j[keep]] = rng.randint(1, 4, keep.sum())
    J = sym(J)
    r = 2000
    J[r, :] = J[:, r] = 0.0
    for c in (0, 63, 64, 127, 128, n - 1):
        J[r, c] = J[c, r] = -3.0
    J[77, :] = J[:, 77] = 0.0  # the empty row
    J[78, 4000] = -0.0         # not an entry
    h = rng.randint(-2, 3, n).astype(np.float32)
    eng.set_field_cache("off")
    eng.set_dense(J, h)
    kind, words = eng.scan_summary()
    rp, ci, v = ref.dense_as_csr(J)
    want = ref.csr_words(rp, ci, v, h)
    q = eng.route_query()
    assert q.from_dense == 1 and q.kind == 1 and kind == 1
    assert words == want, dict(zip(ref.CSR_WORDS, zip(words, want)))
    assert q.nnz == len(ci) and q.max_row_len == want[10] == int((J != 0).sum(1).max())
    c = classify([["csr", n] + words])[0]
    assert (q.acc, q.table_m, q.table_scale, q.clf_ok) == (c["acc"], c["table_m"], c["scale"], c["clf"])
    # the entries themselves: local fields of the all-up state over the reference's conversion
    eng.init_replicas(1, seed=1, s0=np.ones((1, n), np.int8))
    rows = np.asarray([r, 0, 63, 64, 127, 128, n - 1, 77, 78], np.int32)
    prob, up = oracle.Problem(csr=(rp, ci, v), h=h), np.ones(n, np.int8)
    assert np.array_equal(eng.local_fields(0, rows), [oracle.local_field(prob, up, int(i)) for i in rows])


# ----------------------------------------------------------------------------- chains: the class the words chose walks right
CHAINS = [("pm1", "half", 0, 192), ("i127", "128", 191, 192), ("pm1", "2", 63, 64), ("pm1", "asym", 192, 128),
          ("i127", "asym_T", 192, 128), ("grid", "diag", 192, 64), ("pm1", "span52", 64, 128), ("pm1", "span53", 64, 128),
          ("i127", "h_half", 192, 0), ("i127", "h_quarter", 0, 64), ("pm1", "row24_edge", 192, 128), ("pm1", "row24", 192, 128),
          ("pm1", "row15_edge", 63, 127), ("pm1", "row15", 63, 127)]


def walk(e, prob, n, words_consistent, m, tag, seed=11):
    """Two sweeps, three replicas, one at T = inf (every proposal evaluated and accepted), against the oracle."""
    temps = np.asarray([INF, m / 4.0, m / 64.0])
    e.init_replicas(3, seed=seed)
    e.set_temperatures(temps)
    out = e.sweep(2, energy_trace=True)
    s = oracle.init_spins(n, 3, seed)
    want = oracle.sweeps(prob, s, temps, 2, seed=seed, recompute_energy=not words_consistent)
    assert np.array_equal(e.spins(), s), tag
    assert np.array_equal(e.stats()[0], want["n_accepted"]) and want["n_accepted"][0] == 2 * n, tag
    assert np.array_equal(out["energy_trace"], want["energy_trace"]), tag
    assert np.array_equal(e.energies(), want["energy"]), tag


@pytest.mark.parametrize("name,kind,r,c", CHAINS)
def test_dense_chain_of_each_kind_of_plant(eng, name, kind, r, c):
    n = 193
    J, h = plant(*base(name, n), kind, r, c, n)
    eng.set_field_cache("off")
    eng.set_dense(J, h)
    words = eng.scan_summary()[1]
    assert words == ref.dense_words(J, h)
    walk(eng, oracle.Problem(J=J, h=h), n, words[4] == 0, float(np.int32(words[2]).view(np.float32)), (name, kind, eng.describe()))


@pytest.mark.parametrize("name,kind,k", [("pm1", "half", 3), ("i127", "asym", 1), ("pm1", "row15", 2), ("pm1", "row24", 1),
                                         ("grid", "diag", 0), ("pm1", "span53", 2)])
def test_csr_chain_of_each_kind_of_plant(eng, name, kind, k):
    J0, h0 = csr_base(name)
    r, c = csr_positions(J0)[k]  # entry 0 | 63 | 64 | 199 of the 200-entry row
    J, h = plant(J0, h0, kind, r, c, 200, clear=False)
    rp, ci, v = ref.dense_as_csr(J)
    eng.set_field_cache("off")
    eng.set_csr(rp, ci, v, h)
    words = eng.scan_summary()[1]
    assert words == ref.csr_words(rp, ci, v, h)
    walk(eng, oracle.Problem(csr=(rp, ci, v), h=h), len(h), words[4] == 0 and words[5] == 0,
         float(np.int32(words[6]).view(np.float32)), (name, kind, eng.describe()))


# ----------------------------------------------------------------------------- refusals: non-finite values
BAD = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}


def refused_non_finite(sg, call):
    with pytest.raises(sg.AnnealingError, match="non-finite") as err:
        call()
    assert err.value.details["code"] == sg._native.ERR_INVALID


@pytest.mark.parametrize("bad", list(BAD))
def test_dense_setters_refuse_non_finite_values(sg, eng, bad):
    """fmaxf drops a NaN from the row bound and +-Inf equals its own rintf: the scans flag exponent field 255 instead.
    Every position of the plants above, in J and in h; then the engine takes a finite problem as before."""
    x = np.float32(BAD[bad])
    for n, positions in ((193, dense_positions(193) + [(192, 192)]), (1100, LARGE_POSITIONS)):
        J0, h0 = base("i127", n)
        for r, c in positions:
            J = J0.copy()
            J[r, c] = x
            refused_non_finite(sg, lambda: eng.set_dense(J, h0))
        for i in (i for i in (0, 63, 64, 255, 256, n - 1) if i < n):
            h = h0.copy()
            h[i] = x
            refused_non_finite(sg, lambda: eng.set_dense(J0, h))
    n = 193
    Js = np.stack([base("grid", n, seed=s)[0] for s in range(3)])
    hs = np.stack([base("grid", n, seed=s)[1] for s in range(3)])
    for r, c in ((0, n - 1), (n - 1, 128), (63, 64)):
        J = Js.copy()
        J[2, r, c] = x
        refused_non_finite(sg, lambda: eng.set_dense_batch(J, hs))
    for i in (0, n - 1):
        h = hs.copy()
        h[2, i] = x
        refused_non_finite(sg, lambda: eng.set_dense_batch(Js, h))
    with pytest.raises(sg.AnnealingError):
        eng.scan_summary()  # nothing is held after a refusal
    eng.set_dense_batch(Js, hs)
    assert eng.scan_summary()[1] == ref.dense_words(Js, hs)


@pytest.mark.parametrize("bad", list(BAD))
def test_csr_setters_refuse_non_finite_values(sg, eng, bad):
    x = np.float32(BAD[bad])
    J0, h0 = csr_base("i127")
    rp, ci, v = ref.dense_as_csr(J0)
    n = len(h0)
    spots = [int(rp[SPECIAL["deg200"]]) + k for k in (0, 63, 64, 199)] + [0, int(rp[SPECIAL["after_empty"]]), len(ci) - 1]
    for i, k in enumerate(spots):
        v2 = v.copy()
        v2[k] = x
        refused_non_finite(sg, lambda: eng.set_csr(np.asarray(rp, np.int64 if i & 1 else np.int32), ci, v2, h0))
    for i, k in enumerate((0, SPECIAL["empty"], n - 1)):
        h = h0.copy()
        h[k] = x
        refused_non_finite(sg, lambda: eng.set_csr(np.asarray(rp, np.int64 if i & 1 else np.int32), ci, v, h))
    big = ring("pm1", 33000)
    for row, at in ((32768, 0), (32999, 3)):
        p = [a.copy() for a in big]
        p[2][int(p[0][row]) + at] = x
        refused_non_finite(sg, lambda: eng.set_csr(*p))
    p = [a.copy() for a in big]
    p[3][32999] = x
    refused_non_finite(sg, lambda: eng.set_csr(*p))
    first, last = ring("pm1", 70, seed=1), ring("pm1", 45, seed=2)
    for where, k in ((2, len(last[1]) - 1), (2, 0), (3, 44)):
        p = [a.copy() for a in last]
        p[where][k] = x
        with pytest.raises(sg.AnnealingError, match="model 2: non-finite"):
            eng.set_csr_batch([first, (rp, ci, v, h0), tuple(p)])
    eng.set_csr(rp, ci, v, h0)
    assert eng.scan_summary()[1] == ref.csr_words(rp, ci, v, h0)


# ----------------------------------------------------------------------------- refusals: structure
# Each defect is refused before anything is read through it: csr_check_rowptr_kernel reads the extents only and runs
# before any entry is touched; csr_scan_kernel compares a column, never follows it, and runs before csr_symmetry_kernel
# and the diagonal gather do.
def set_batch_raw(sg, e, sizes, rp, ci, v, h):
    sizes = np.ascontiguousarray(sizes, np.int32)
    rp, ci = np.ascontiguousarray(rp, np.int64), np.ascontiguousarray(ci, np.int32)
    v, h = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(h, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = e._lib.sga_set_csr_batch(e._h, int(sizes.size), ptr(sizes), ptr(rp), ptr(ci), ptr(v), ptr(h), int(ci.size))
    return rc, sg._native.last_error()


def test_bad_row_extents_are_refused_by_every_csr_setter(sg, eng):
    J0, h0 = csr_base("pm1")
    rp, ci, v = ref.dense_as_csr(J0)
    n, nnz = len(h0), len(ci)
    mid = SPECIAL["deg200"]
    defects = {"rowptr[0] = 1": (0, 1), "rowptr[n] = nnz + 1": (n, nnz + 1), "rowptr[n] = nnz - 1": (n, nnz - 1),
               "row 0 ends below its start": (1, -1), "step down behind row 0": (1, int(rp[2]) + 1),
               "row n - 1 starts behind its end": (n - 1, nnz + 1), "step down into row n - 1": (n - 1, int(rp[n - 2]) - 1),
               "negative extent": (mid, -3), "middle extent above nnz": (mid, nnz + 5)}
    first = ring("pm1", 70, seed=1)
    from spin_glass_anneal_rl_amd.engine import concat_csr_batch
    for what, (k, value) in defects.items():
        bad = np.asarray(rp, np.int64).copy()
        bad[k] = value
        assert ref.csr_words(bad, ci, v, h0) == [1], what
        for dtype in (np.int32, np.int64):
            with pytest.raises(sg.AnnealingError, match="CSR rowptr is not monotone or does not span") as err:
                eng.set_csr(bad.astype(dtype), ci, v, h0)
            assert err.value.details["code"] == sg._native.ERR_INVALID, what
        sizes, brp, bci, bv, bh = concat_csr_batch([first, first, (rp, ci, v, h0)])
        brp[2 * 70 + k] = value + (brp[2 * 70] if value >= 0 or k == 0 else 0)  # the defect, in the last model's extents
        if what == "rowptr[0] = 1":
            continue  # (a batch's model 2 has no rowptr[0] of its own: its first extent is model 1's last)
        rc, msg = set_batch_raw(sg, eng, sizes, brp, bci, bv, bh)
        assert rc == sg._native.ERR_INVALID and "CSR batch rowptr is not monotone or does not span" in msg, (what, rc, msg)
    eng.set_csr(rp, ci, v, h0)
    assert eng.scan_summary()[1] == ref.csr_words(rp, ci, v, h0)


def test_bad_columns_are_refused_by_every_csr_setter(sg, eng):
    J0, h0 = csr_base("pm1")
    rp, ci, v = ref.dense_as_csr(J0)
    n = len(h0)
    first = ring("pm1", 70, seed=1)
    from spin_glass_anneal_rl_amd.engine import concat_csr_batch
    sizes, brp, bci, bv, bh = concat_csr_batch([first, first, (rp, ci, v, h0)])
    spots = [int(rp[SPECIAL["deg200"]]) + k for k in (0, 63, 64)] + [0, len(ci) - 1, int(rp[n - 1])]
    for k in spots:
        for col in (-1, n):
            bad = ci.copy()
            bad[k] = col
            assert ref.csr_words(rp, bad, v, h0) == [0, 1]
            for dtype in (np.int32, np.int64):
                with pytest.raises(sg.AnnealingError, match="CSR column index out of range") as err:
                    eng.set_csr(np.asarray(rp, dtype), bad, v, h0)
                assert err.value.details["code"] == sg._native.ERR_INVALID
            bbad = bci.copy()
            bbad[2 * len(first[1]) + k] = col
            rc, msg = set_batch_raw(sg, eng, sizes, brp, bbad, bv, bh)
            assert rc == sg._native.ERR_INVALID and f"model 2: CSR column index out of range [0, {n})" in msg, (k, col, rc, msg)
    eng.set_csr_batch([first, first, (rp, ci, v, h0)])
    assert eng.scan_summary(2)[1] == ref.csr_words(rp, ci, v, h0)
