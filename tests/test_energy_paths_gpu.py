"""From-scratch energies on every energy path, pinned to an exact reference (tests/exact_energy.py).

Every replica is given the same spins (init_replicas(..., s0=...)), so every energy of a launch must be the same,
whatever kernel recomputed it:
  a. integer and narrow-range dyadic problems: every path, every replica count and every batched_energy setting
     equals `contract_energy` (the documented rounding chain on exact sums) bit for bit;
  b. under the default batched_energy = 1 a replica's energy carries the same bits for every problem class across
     replica counts, set_spins / init_replicas / recompute_energies, sharded and unsharded engines, the field cache
     and the scratch tiling of the all-replica pass;
  c. Gaussian and wide-range problems: every path, batched_energy = 2 included, lies within `energy_bound` of the
     exact energy.
The counts cover the thresholds of recompute_energy_range: the slice formula (1 .. 511), one workgroup per replica
(512+), the matrix-core pass (32+) and the CSR all-replica pass (64+)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import exact_energy as xe  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS = [1, 6, 31, 32, 63, 64, 96, 300, 400, 511, 512, 600]


def _sg():
    import spin_glass_anneal_rl_amd as sg
    return sg


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def _spins(seed, n):
    return np.where(np.random.RandomState(seed).random_sample(n) < 0.5, -1, 1).astype(np.int8)


def _energies(setup, s, R, batched=1, options=None, R_global=None, replica0=0):
    """Energies of R replicas that all hold spins s, straight from init_replicas."""
    sg = _sg()
    with sg.AnnealEngine(0) as e:
        for k, v in dict(options or {}, batched_energy=batched).items():
            e.set_option(k, v)
        setup(e)
        e.init_replicas(R, seed=7, s0=np.tile(s, (R, 1)), R_global=R_global, replica0=replica0)
        return e.energies()


def _all_equal(E, what):
    E = np.asarray(E)
    bad = np.nonzero(_bits(E) != _bits(E[:1]))[0]
    assert bad.size == 0, f"{what}: replica {bad[0]} has {E[bad[0]]!r}, replica 0 {E[0]!r}"
    return float(E[0])


# ---------------------------------------------------------------------------------------------------------------
# dense problems: (J, h, storage, kind), kind "exact" (a) or "bound" (c)
# ---------------------------------------------------------------------------------------------------------------
def _dense(J, h, storage="auto"):
    def setup(e):
        e.set_dense(np.asarray(J, np.float32), np.asarray(h, np.float32), storage=storage)
    return setup


def _int_row_2p24(n, v):
    """Integer J: row 0 / column 0 of +-v, +v in the first 60 % of the columns, +-1 elsewhere.  At all spins +1 (what
    the tests give these problems) the k-order partial sums of row 0 climb to ~0.6 n v before coming back to
    ~0.2 n v: past 2^24 for v = 65537, below it for v = 32767."""
    rng = np.random.RandomState(v)
    A = rng.randint(-1, 2, (n, n)).astype(np.float64)
    A[0, 1:] = np.where(np.arange(1, n) < 0.6 * n, v, -v)
    return xe.sym(A), (rng.randint(-3, 4, n) / 2.0).astype(np.float32)


def _dense_problems():
    rng = np.random.RandomState(1)
    n = 300
    P = {}
    P["pm1_f32"] = (xe.sym(rng.randint(-1, 2, (n, n))), rng.randint(-2, 3, n).astype(np.float32), "f32", "exact")
    P["pm1_t2"] = (P["pm1_f32"][0], P["pm1_f32"][1], "t2", "exact")
    P["int127_i8"] = (xe.sym(rng.randint(-127, 128, (n, n))), np.zeros(n, np.float32), "i8", "exact")
    J128 = xe.sym(rng.randint(-127, 128, (n, n)))
    J128[3, 4] = J128[4, 3] = 128.0  # max |J| = 128: no int8 storage, the f32 kinds
    P["int128"] = (J128, np.zeros(n, np.float32), "auto", "exact")
    # a row sum of |J| just below 2^24 (fp32 class) and at it (f64 matrix-core mode); the second with odd entries
    P["row_below_2p24"] = (*_int_row_2p24(512, 32767), "auto", "exact")
    P["row_at_2p24"] = (*_int_row_2p24(512, 65537), "auto", "exact")
    P["half_h"] = (xe.sym(rng.randint(-3, 4, (n, n))), (rng.randint(-7, 8, n) / 2.0).astype(np.float32), "auto",
                   "exact")
    # dyadic reals of a narrow binary range: row sums, X and Y all exact in fp64 (f64-exact class)
    P["dyadic"] = (xe.sym(rng.randint(-255, 256, (n, n)) / 64.0), (rng.randint(-31, 32, n) / 8.0).astype(np.float32),
                   "auto", "exact")
    P["gauss"] = (xe.sym(np.random.RandomState(2).standard_normal((1000, 1000))),
                  np.random.RandomState(3).standard_normal(1000).astype(np.float32), "auto", "bound")
    Jw, hw = xe.witness_dense()
    P["witness"] = (Jw, hw, "auto", "bound")
    # the cancellation moved across block (8-row), slice and wave-chain boundaries
    P["witness_blocks"] = (*xe.witness_dense(300, 7, 8, 255, 256, 120, 121), "auto", "bound")
    P["witness_3000"] = (*xe.witness_dense(3000, 11, 12, 2999, 1500, 1497, 1498), "auto", "bound")
    # f64-exact class (row sums exact in any order) whose X is not exact in fp64: the batched passes must add X in
    # the per-replica kernels' order to give their bits (n = 1024: the 1 MB scratch below forms tiles)
    P["f64_inexact_x"] = (*xe.f64_inexact_x(1024), "auto", "bound")
    return P


DENSE = _dense_problems()
SPARSE_ROUTE_OFF = {"sparse_route": 0}
ONES = ("witness", "row_", "f64_inexact")  # problems built for all spins +1


def _spins_of(name, n, seed):
    return np.ones(n, np.int8) if name.startswith(ONES) else _spins(seed, n)


def _reference(s, J, h, kind, rows):
    if kind == "exact":
        return xe.contract_energy(s, h, J=J, rows=rows), None
    return xe.energy_bound(s, h, J=J, rows=rows)


def _check(name, v, ref, kind):
    if kind == "exact":
        assert _bits(v) == _bits(ref[0]), f"{name}: energy {v!r} != contract {ref[0]!r}"
    else:
        assert abs(v - ref[0]) <= ref[1], f"{name}: |E - E*| = {abs(v - ref[0])!r} > bound {ref[1]!r} (E* {ref[0]!r})"


@pytest.mark.parametrize("name", sorted(DENSE))
def test_dense_every_count(name):
    J, h, storage, kind = DENSE[name]
    n = J.shape[0]
    s = _spins_of(name, n, 5)
    ref = _reference(s, J, h, kind, xe.Rows(J=J))
    setup = _dense(J, h, storage)
    at1 = {}
    for batched in (1, 0, 2):
        for R in COUNTS:
            E = _energies(setup, s, R, batched, SPARSE_ROUTE_OFF)
            e0 = _all_equal(E, f"{name} R={R} batched={batched}")
            at1.setdefault(batched, {})[R] = e0
            _check(f"{name} R={R} batched={batched}", e0, ref, kind)
    # b: under the default, one value whatever the count
    e1 = at1[1][1]
    for R, v in at1[1].items():
        assert _bits(v) == _bits(e1), f"{name}: R={R} gives {v!r}, R=1 gives {e1!r} (batched_energy=1)"


def test_witness_count_independent():
    """The issue's witness: the per-replica kernel at 1..600 replicas (8, 6, 4, 3 and 1 slices before)."""
    J, h = xe.witness_dense()
    s = np.ones(64, np.int8)
    for R in COUNTS:
        E = _energies(_dense(J, h), s, R, 1, SPARSE_ROUTE_OFF)
        assert _all_equal(E, f"R={R}") == -1.0, f"R={R}: {E[0]!r}"
    for R in (1, 200, 400, 600):  # left to the sparse route: energy_csr_kernel, the same slice formula before
        E = _energies(_dense(J, h), s, R, 1)
        assert _all_equal(E, f"sparse route R={R}") == -1.0, f"sparse route R={R}: {E[0]!r}"


@pytest.mark.parametrize("name", ["pm1_f32", "dyadic", "gauss", "witness_blocks", "f64_inexact_x"])
def test_recompute_paths_agree(name):
    """set_spins (one replica), recompute_energies, a shard of a larger run, the field cache and a 1 MB scratch
    for the all-replica pass (f64_inexact_x, n = 1024: tiles of 256 replicas at R = 600): the bits of
    init_replicas at R = 1."""
    sg = _sg()
    J, h, storage, kind = DENSE[name]
    n = J.shape[0]
    s = _spins_of(name, n, 9)
    ref = _all_equal(_energies(_dense(J, h, storage), s, 1, 1, SPARSE_ROUTE_OFF), "R=1")
    for R, opts in ((600, {"fields_scratch_mb": 1}), (96, {})):
        with sg.AnnealEngine(0) as e:
            for k, v in dict(SPARSE_ROUTE_OFF, **opts).items():
                e.set_option(k, v)
            _dense(J, h, storage)(e)
            other = np.where(np.arange(n) % 3 == 0, -1, 1).astype(np.int8)
            e.init_replicas(R, seed=3, s0=np.tile(other, (R, 1)))
            for r in (0, R // 2, R - 1):
                e.set_spins(r, s)
                assert _bits(e.energies()[r]) == _bits(ref), f"{name}: set_spins({r}) at R={R}"
            e.init_replicas(R, seed=3, s0=np.tile(s, (R, 1)))
            for mode in ("on", "off"):
                e.set_field_cache(mode)
                e.recompute_energies()
                assert _bits(_all_equal(e.energies(), f"recompute R={R} cache={mode}")) == _bits(ref)
    for R_local, Rg, r0 in ((6, 12, 6), (300, 600, 300), (64, 640, 576)):
        E = _energies(_dense(J, h, storage), s, R_local, 1, SPARSE_ROUTE_OFF, R_global=Rg, replica0=r0)
        assert _bits(_all_equal(E, f"shard {r0}+{R_local} of {Rg}")) == _bits(ref), f"{name}: shard {r0} of {Rg}"


def test_dense_batch_many_models():
    rng = np.random.RandomState(4)
    M, n = 3, 200
    Js = [xe.sym(rng.randint(-5, 6, (n, n))) for _ in range(M)]
    hs = [(rng.randint(-3, 4, n) / 2.0).astype(np.float32) for _ in range(M)]
    Jg = [xe.sym(rng.standard_normal((n, n))) for _ in range(M)]
    s = _spins(8, n)
    sg = _sg()
    for Jm, exact in ((Js, True), (Jg, False)):
        want = []
        for m in range(M):
            if exact:
                want.append(xe.contract_energy(s, hs[m], J=Jm[m]))
            else:
                want.append(xe.energy_bound(s, hs[m], J=Jm[m]))
        per_model = {}
        for R in (3, 6, 96, 600):
            with sg.AnnealEngine(0) as e:
                e.set_dense_batch(np.stack(Jm), np.stack(hs))
                e.init_replicas(R, seed=1, s0=np.tile(s, (R, 1)))
                E = e.energies()
            for m in range(M):
                Em = E[m * (R // M):(m + 1) * (R // M)]
                v = _all_equal(Em, f"model {m} R={R}")
                per_model.setdefault(m, set()).add(int(_bits(v)))
                if exact:
                    assert _bits(v) == _bits(want[m]), f"model {m} R={R}: {v!r} != {want[m]!r}"
                else:
                    assert abs(v - want[m][0]) <= want[m][1], f"model {m} R={R}"
        assert all(len(b) == 1 for b in per_model.values()), per_model


def _pairs_csr_example():
    """n = 64, f64-exact class (span 52, one entry per row) with X not exact: +2^30 on (0,1) .. (6,7), 2^-21 on
    (8,9), -2^30 on (16,17) .. (22,23)."""
    n = 64
    J = np.zeros((n, n), np.float32)
    pairs = [(2 * k, 2 * k + 1, 2.0 ** 30) for k in range(4)] + [(8, 9, 2.0 ** -21)]
    pairs += [(16 + 2 * k, 17 + 2 * k, -2.0 ** 30) for k in range(4)]
    for a, b, v in pairs:
        J[a, b] = J[b, a] = v
    return J, np.zeros(n, np.float32)


@pytest.mark.parametrize("name", ["f64_inexact_x", "pairs"])
@pytest.mark.parametrize("form", ["dense", "csr"])
def test_f64_class_inexact_x_every_count(name, form):
    """Row sums exact in fp64 in any order, X not: under batched_energy = 1 the matrix-core pass (dense, 32+
    replicas) and the CSR all-replica pass (64+; only where X is provably exact) must give the per-replica kernels'
    bits at every count; every setting stays within the bound."""
    J, h = xe.f64_inexact_x(1024) if name == "f64_inexact_x" else _pairs_csr_example()
    n = J.shape[0]
    s = np.ones(n, np.int8)
    p = xe.exact_parts(s, h, J=J)
    assert xe.canonical_x(p["mv"], s) != float(p["X"]), "X must not be exact in fp64 for this problem"
    ref = xe.energy_bound(s, h, J=J)
    if form == "dense":
        setup, opts = _dense(J, h), SPARSE_ROUTE_OFF
    else:
        csr = xe.dense_to_csr(J)
        setup, opts = (lambda e: e.set_csr(*csr, h)), {}
    at1 = {}
    for batched in (1, 0, 2):
        for R in COUNTS:
            v = _all_equal(_energies(setup, s, R, batched, opts), f"{name} {form} R={R} batched={batched}")
            _check(f"{name} {form} R={R} batched={batched}", v, ref, "bound")
            if batched == 1:
                at1[R] = v
    for R, v in at1.items():
        assert _bits(v) == _bits(at1[1]), f"{name} {form}: R={R} gives {v!r}, R=1 gives {at1[1]!r}"


# ---------------------------------------------------------------------------------------------------------------
# CSR
# ---------------------------------------------------------------------------------------------------------------
def _sparse_J(n, deg, seed, kind):
    rng = np.random.RandomState(seed)
    i = rng.randint(0, n, n * deg)
    j = rng.randint(0, n, n * deg)
    keep = i != j
    i, j = i[keep], j[keep]
    if kind == "int":
        v = rng.randint(-9, 10, i.size).astype(np.float64)
    elif kind == "dyadic":
        v = rng.randint(-255, 256, i.size) / 32.0
    elif kind == "gauss":
        v = rng.standard_normal(i.size)
    else:  # wide: many binary decades apart
        v = rng.standard_normal(i.size) * 2.0 ** rng.randint(-40, 41, i.size)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    key = lo.astype(np.int64) * n + hi
    key, first = np.unique(key, return_index=True)
    lo, hi, v = lo[first], hi[first], v[first].astype(np.float32)
    r = np.concatenate([lo, hi])
    c = np.concatenate([hi, lo])
    vv = np.concatenate([v, v])
    order = np.lexsort((c, r))
    r, c, vv = r[order], c[order], vv[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
    return rowptr, c.astype(np.int32), vv


@pytest.mark.parametrize("kind", ["int", "dyadic", "gauss", "wide"])
def test_csr_every_count(kind):
    n = 3000
    csr = _sparse_J(n, 8, 21, kind)
    rng = np.random.RandomState(22)
    h = (rng.randint(-5, 6, n) / 2.0).astype(np.float32) if kind in ("int", "dyadic") else \
        rng.standard_normal(n).astype(np.float32)
    s = _spins(23, n)
    rows = xe.Rows(csr=csr)
    setup = lambda e: e.set_csr(*csr, h)  # noqa: E731
    exact = kind in ("int", "dyadic")
    want = xe.contract_energy(s, h, rows=rows) if exact else None
    Ex, B = (None, None) if exact else xe.energy_bound(s, h, rows=rows)
    at1 = {}
    for batched in (1, 0, 2):
        for R in COUNTS:
            v = _all_equal(_energies(setup, s, R, batched), f"csr {kind} R={R} batched={batched}")
            if batched == 1:
                at1[R] = v
            if exact:
                assert _bits(v) == _bits(want), f"csr {kind} R={R} batched={batched}: {v!r} != {want!r}"
            else:
                assert abs(v - Ex) <= B, f"csr {kind} R={R} batched={batched}: {v!r}, E* {Ex!r} bound {B!r}"
    assert len({int(_bits(v)) for v in at1.values()}) == 1, at1


@pytest.mark.parametrize("kind,n", [("int", 200_000), ("gauss", 200_000), ("int", 200_064), ("gauss", 200_064)])
def test_csr_large_n(kind, n):
    """Spins beyond the int8 LDS capacity: from HBM (n = 200 000) or as bits in LDS (n = 200 064, a multiple of
    128)."""
    csr = _sparse_J(n, 3, 31, kind)
    h = (np.random.RandomState(32).randint(-3, 4, n) / 2.0).astype(np.float32)
    s = _spins(33, n)
    rows = xe.Rows(csr=csr)
    setup = lambda e: e.set_csr(*csr, h)  # noqa: E731
    vals = {}
    for R in (1, 6, 64, 512):
        vals[R] = _all_equal(_energies(setup, s, R, 1), f"R={R}")
    assert len({int(_bits(v)) for v in vals.values()}) == 1, vals
    if kind == "int":
        assert _bits(vals[1]) == _bits(xe.contract_energy(s, h, rows=rows))
    else:
        Ex, B = xe.energy_bound(s, h, rows=rows)
        assert abs(vals[1] - Ex) <= B


def test_ragged_batch():
    sg = _sg()
    sizes = (150, 333, 64)
    probs_int = []
    probs_g = []
    for k, n in enumerate(sizes):
        rp, ci, v = _sparse_J(n, 6, 40 + k, "int")
        probs_int.append((rp, ci, v, (np.random.RandomState(k).randint(-3, 4, n) / 2.0).astype(np.float32)))
        rp, ci, v = _sparse_J(n, 6, 50 + k, "gauss")
        probs_g.append((rp, ci, v, np.random.RandomState(k).standard_normal(n).astype(np.float32)))
    for probs, exact in ((probs_int, True), (probs_g, False)):
        for R in (3, 6, 96, 600):
            with sg.AnnealEngine(0) as e:
                e.set_csr_batch(probs)
                e.init_replicas(R, seed=11)
                E = e.energies()
                for r in sorted({0, R // 3, R // 2, R - 1}):
                    m = r // (R // len(sizes))
                    rp, ci, v, h = probs[m]
                    s = e.spins(r)
                    if exact:
                        want = xe.contract_energy(s, h, csr=(rp, ci, v))
                        assert _bits(E[r]) == _bits(want), f"ragged R={R} r={r}: {E[r]!r} != {want!r}"
                    else:
                        Ex, B = xe.energy_bound(s, h, csr=(rp, ci, v))
                        assert abs(E[r] - Ex) <= B, f"ragged R={R} r={r}"
                    e.set_spins(r, s)
                    assert _bits(e.energies()[r]) == _bits(E[r]), f"ragged set_spins R={R} r={r}"


def test_tsp_energies():
    sg = _sg()
    import spin_glass_anneal_rl_amd.encoders as enc
    rng = np.random.RandomState(60)
    nc = 12
    d = rng.randint(1, 90, (nc, nc)).astype(np.float64)
    d = np.triu(d, 1) + np.triu(d, 1).T
    rowptr, colidx, val, h, _ = enc.tsp_csr(d)
    csr = (rowptr.numpy(), colidx.numpy(), val.numpy())
    h = h.numpy()
    dist, cv, pf, hs, _ = enc.tsp_structure(d)
    s = _spins(61, nc * nc)
    want = xe.contract_energy(s, h, csr=csr)
    vals = {}
    for batched in (1, 2):
        for R in (1, 6, 64, 300, 512, 600):
            E = _energies(lambda e: e.set_tsp(dist, cv, pf, hs), s, R, batched)
            vals[(batched, R)] = v = _all_equal(E, f"tsp R={R}")
            assert _bits(v) == _bits(want), f"tsp R={R} batched={batched}: {v!r} != {want!r}"


def test_asymmetric_trace_same_at_6_and_600():
    """Asymmetric real J: the energy is recomputed from scratch after every sweep.  The followed replicas run the
    same chains at R = 6 and R = 600, so their traces must carry the same bits."""
    sg = _sg()
    n = 257
    rng = np.random.RandomState(70)
    J = rng.standard_normal((n, n)).astype(np.float32)
    np.fill_diagonal(J, 0.0)
    h = rng.standard_normal(n).astype(np.float32)
    traces = {}
    for R in (6, 600):
        with sg.AnnealEngine(0) as e:
            e.set_dense(J, h)
            e.init_replicas(R, seed=5)
            e.set_temperatures(np.full(R, 1.5))
            traces[R] = e.sweep(4, energy_trace=True)["energy_trace"][:, :6].copy()
            final = e.spins()[:6]
    np.testing.assert_array_equal(_bits(traces[6]), _bits(traces[600]))
    for r in range(6):
        Ex, B = xe.energy_bound(final[r], h, J=J)
        assert abs(traces[600][-1, r] - Ex) <= B
