"""Simulated quantum annealing on the device (sga_sweep_transverse, csrc/sweep_transverse.hip) against the plain-Python
specification of tests/transverse_reference.py: spins, energies, bests and accept counters bit for bit (np.array_equal),
on 3^3 and 6^3 periodic +-J lattices and a random graph of 300 sites (degree ~8, |J| <= 5, half-integer h, one empty row),
P in {2, 4, 6} slices x G in {1, 3} groups at distinct temperatures per group, both arithmetics, 3 sweeps.  The reference
runs of a shape are computed once per case and shared."""
import functools

import numpy as np
import pytest
import torch

import groups_cases as gc
import oracle
import transverse_reference as tr
from test_cluster_moves_gpu import SEED, csr_from_edges, pm, state

pytestmark = pytest.mark.gpu

NS = 3
PG = [(2, 1), (2, 3), (4, 1), (4, 3), (6, 1), (6, 3)]
ARITHS = [oracle.ARITH_F64, oracle.ARITH_F32]


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def lattice3d(L, rng):
    idx = lambda x, y, z: ((x % L) * L + (y % L)) * L + (z % L)  # noqa: E731
    return csr_from_edges(L ** 3, [(idx(x, y, z), idx(x + dx, y + dy, z + dz), pm(rng)) for x in range(L) for y in range(L)
                                   for z in range(L) for dx, dy, dz in ((1, 0, 0), (0, 1, 0), (0, 0, 1))])


def random300(rng):
    n, edges = 300, {}
    for i in range(n - 1):
        for j in rng.choice(n - 1, 4, replace=False):  # site n - 1 has no bond: an empty row
            if i != j:
                edges[(min(i, j), max(i, j))] = float(rng.choice([-5, -4, -3, -2, -1, 1, 2, 3, 4, 5]))
    return csr_from_edges(n, [(i, j, v) for (i, j), v in sorted(edges.items())])


@functools.lru_cache(maxsize=None)
def shape(name):
    """(graph, h) of a shape, made once."""
    rng = np.random.RandomState({"lattice3": 3, "lattice6": 6, "random300": 300}[name])
    if name == "lattice3":
        g = lattice3d(3, rng)
        return g, np.zeros(27, np.float32)
    if name == "lattice6":
        g = lattice3d(6, rng)
        return g, rng.randint(-1, 2, 216).astype(np.float32)
    g = random300(rng)
    assert g[0][300] == g[0][299] and 7.0 < g[0][300] / 300 < 8.5
    return g, (rng.randint(-3, 4, 300) / 2.0).astype(np.float32)


SHAPES = ["lattice3", "lattice6", "random300"]


def temps(P, G):
    return np.repeat(1.5 + 0.7 * np.arange(G), P)  # equal within a group, distinct between groups


def couplings(G):
    """A different k per sweep and per group, out of {0.25, 5, -1}."""
    vals = np.asarray([0.25, 5.0, -1.0], np.float32)
    return vals[(np.arange(NS)[:, None] + np.arange(G)[None, :]) % 3]


def engine(sg, name, R, T, cache=None, seed=SEED, s0=None, **replicas):
    g, h = shape(name)
    e = sg.AnnealEngine(0)
    if cache is not None:
        e.set_field_cache(cache)
    e.set_csr(*g, h)
    e.init_replicas(R, seed=seed, s0=s0, **replicas)
    e.set_temperatures(T)
    return e


def reference(name, P, G, arith, k, T=None, ns=NS, s0=None, seed=SEED, replica0=0):
    g, h = shape(name)
    prob = oracle.Problem(csr=g, h=h)
    S = oracle.init_spins(prob.n, P * G, seed, replica0=replica0) if s0 is None else s0.copy()
    out = tr.sweeps(prob, S, temps(P, G) if T is None else T, ns, P, k, arith=arith, seed=seed, replica0=replica0)
    return S, out


def assert_matches(e, S, out):
    st = state(e)
    assert np.array_equal(st["S"], S)
    assert np.array_equal(st["E"], out["energy"])
    assert np.array_equal(st["acc"], out["n_accepted"])
    assert np.array_equal(st["be"], out["best_energy"])
    assert np.array_equal(st["bs"], out["best_spins"])


def assert_same_state(a, b):
    for key in ("S", "E", "acc", "be", "bs"):
        assert np.array_equal(a[key], b[key]), key


# ---- 1. k = 0 is sga_sweep, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("P,G", PG)
@pytest.mark.parametrize("name", SHAPES)
def test_k_zero_is_the_plain_sweep(sg, name, P, G, arith):
    T = temps(P, G)
    with engine(sg, name, P * G, T) as e, engine(sg, name, P * G, T) as twin:
        e.sweep_transverse(NS, P, 0.0, arith=arith)
        twin.sweep(NS, arith=arith)
        assert_same_state(state(e), state(twin))
        assert state(e)["acc"].sum() > 0
        assert e.counters() == twin.counters()


# ---- 2. against the reference, a different k per sweep and group -----------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("P,G", PG)
@pytest.mark.parametrize("name", SHAPES)
def test_against_the_reference(sg, name, P, G, arith):
    k = couplings(G)
    S, out = reference(name, P, G, arith, k)
    with engine(sg, name, P * G, temps(P, G)) as e:
        e.sweep_transverse(NS, P, k, arith=arith)
        assert_matches(e, S, out)
        assert out["n_accepted"].sum() > 0
        # 7. the tracked energies are the classical ones
        E = e.energies()
        e.recompute_energies()
        assert np.array_equal(e.energies(), E)
        g, h = shape(name)
        assert np.array_equal(E, [oracle.energy(oracle.Problem(csr=g, h=h), r) for r in S])


# ---- 3. one call of 2 sweeps equals two calls of 1 sweep -------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name,P,G", [("lattice3", 2, 3), ("lattice6", 4, 3), ("random300", 6, 1)])
def test_two_sweeps_are_two_calls(sg, name, P, G, arith):
    k = couplings(G)[:2]
    T = temps(P, G)
    with engine(sg, name, P * G, T) as e, engine(sg, name, P * G, T) as twin:
        e.sweep_transverse(2, P, k, arith=arith)
        twin.sweep_transverse(1, P, k[:1], arith=arith)
        twin.sweep_transverse(1, P, k[1:], arith=arith)
        assert_same_state(state(e), state(twin))
        assert e.counters() == twin.counters() == (2, 0)


# ---- 4. a rank that holds whole groups --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,P", [("lattice3", 2), ("lattice6", 6), ("random300", 4)])
def test_sharded_groups(sg, name, P):
    G, k = 3, couplings(3)
    T = temps(P, G)
    with engine(sg, name, P * G, T) as full:
        full.sweep_transverse(NS, P, k)
        want = state(full)
    for g0, gn in ((1, 2), (2, 1)):  # the last two groups, the last one
        lo, R = g0 * P, gn * P
        with engine(sg, name, R, T[lo:], R_global=P * G, replica0=lo) as part:
            part.sweep_transverse(NS, P, k[:, g0:])
            got = state(part)
            for key in ("S", "E", "acc", "be", "bs"):
                assert np.array_equal(got[key], want[key][lo:lo + R]), key


# ---- 5. T = 0 and T = inf ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name,P", [("lattice6", 4), ("random300", 2)])
def test_temperature_limits(sg, name, P, arith):
    G = 3
    T = np.repeat([0.0, np.inf, 1.0], P)
    k = couplings(G)
    S, out = reference(name, P, G, arith, k, T=T)
    with engine(sg, name, P * G, T) as e:
        e.sweep_transverse(NS, P, k, arith=arith)
        assert_matches(e, S, out)
    n = S.shape[1]
    assert np.all(out["n_accepted"][P:2 * P] == NS * n)  # T = inf accepts everything
    assert np.all(out["n_accepted"][:P] < NS * n)


# ---- 6. identical slices under a large coupling are frozen ---------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name,P,G", [("lattice3", 2, 1), ("lattice6", 6, 3), ("random300", 4, 3)])
def test_frozen_slices(sg, name, P, G, arith):
    n = len(shape(name)[1])
    s0 = np.repeat(oracle.init_spins(n, 1, SEED), P * G, axis=0)
    with engine(sg, name, P * G, 1.0, s0=s0) as e:
        before = state(e)
        e.sweep_transverse(NS, P, 1.0e4, arith=arith)
        after = state(e)
        assert np.array_equal(after["S"], s0) and not after["acc"].any()
        assert_same_state(before, after)


# ---- 8. what moves and what does not -------------------------------------------------------------------------------------------
def test_counters_ladder_and_exchange_statistics(sg):
    name, P, G = "lattice6", 4, 3
    with engine(sg, name, P * G, 1.0) as e:
        e.set_ladder(np.tile([0.5, 1.0, 2.0, 4.0], G), n_ladders=G)
        e.sweep(2)
        e.exchange()
        e.exchange()
        slot, stats, T = e.slot_map(), e.exchange_stats(), e.temperatures()
        assert stats[0].sum() > 0 and e.counters() == (2, 2)
        e.sweep_transverse(NS, P, 0.25)
        assert e.counters() == (2 + NS, 2)
        assert np.array_equal(e.slot_map(), slot) and np.array_equal(e.temperatures(), T)
        assert all(np.array_equal(a, b) for a, b in zip(e.exchange_stats(), stats))
        assert np.array_equal(e.stats()[1], np.full(P * G, (2 + NS) * 216))
        assert "sweep_transverse_kernel" in e.last_kernel()
        e.sweep_transverse(0, P, 0.25)  # a no-op
        assert e.counters() == (2 + NS, 2)


# ---- 9. the cached fields are seeded anew --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice3", "lattice6"])
def test_field_cache_is_reseeded(sg, name):
    P, G = 4, 3
    T = temps(P, G)
    with engine(sg, name, P * G, T, cache="on") as e, engine(sg, name, P * G, T, cache="on") as twin:
        e.sweep(1)
        twin.sweep(1)
        assert "sweep_clf_csr_kernel" in e.last_kernel()  # the fields are resident and valid now
        e.sweep_transverse(2, P, couplings(G)[:2])
        mid = state(e)
        for r in range(P * G):
            twin.set_spins(r, mid["S"][r])
        twin.set_counters(*e.counters())
        assert np.array_equal(twin.energies(), mid["E"])
        e.sweep(2)
        twin.sweep(2)
        assert "sweep_clf_csr_kernel" in e.last_kernel()
        a, b = state(e), state(twin)
        assert np.array_equal(a["S"], b["S"]) and np.array_equal(a["E"], b["E"])
        e.recompute_energies()
        assert np.array_equal(e.energies(), a["E"])


# ---- 10. refusals leave the engine as it was --------------------------------------------------------------------------------------
def refused(sg, e, code, word, *args, **kw):
    ragged = getattr(e, "_sizes", None) is not None  # (best(r) of a ragged batch has the model's own length)
    before = dict(S=e.spins(), E=e.energies(), acc=e.stats()[0]) if ragged else state(e)
    counters = e.counters()
    with pytest.raises(sg.AnnealingError) as err:
        e.sweep_transverse(*args, **kw)
    assert err.value.details["code"] == code and word in str(err.value), str(err.value)
    now = dict(S=e.spins(), E=e.energies(), acc=e.stats()[0]) if ragged else state(e)
    assert all(np.array_equal(now[key], before[key]) for key in before)
    assert e.counters() == counters


def test_invalid_calls(sg):
    N = sg._native
    with engine(sg, "lattice3", 12, 1.0) as e:
        e.sweep(1)
        for P in (1, 0, -2, 3, 5, 8, 24):
            refused(sg, e, N.ERR_INVALID, "n_slices", 1, P, 0.25)
        refused(sg, e, N.ERR_INVALID, "n_sweeps", -1, 4, 0.25)
        refused(sg, e, N.ERR_INVALID, "arith", 1, 4, 0.25, arith=7)
        for bad in (np.nan, np.inf, -np.inf, [[0.25, 0.25, np.nan]]):
            refused(sg, e, N.ERR_INVALID, "k_perp", 1, 4, bad)
        assert N.lib().sga_sweep_transverse(e._h, 1, 4, N.ARITH_F64, None) == N.ERR_INVALID
        k = np.zeros(3, np.float32)
        assert N.lib().sga_sweep_transverse(None, 1, 4, N.ARITH_F64, k.ctypes.data) == N.ERR_INVALID
        dev = torch.zeros(3, dtype=torch.float32, device="cuda")
        assert N.lib().sga_sweep_transverse(e._h, 1, 4, N.ARITH_F64, dev.data_ptr()) == N.ERR_INVALID
        assert e.counters() == (1, 0)
    with engine(sg, "lattice3", 8, 1.0, R_global=16, replica0=6) as e:  # replica0 % 4 != 0
        refused(sg, e, N.ERR_INVALID, "replica0", 1, 4, 0.25)
        e.sweep_transverse(1, 2, 0.25)  # 6 % 2 == 0
    g, h = shape("lattice3")
    with sg.AnnealEngine(0) as e:
        with pytest.raises(sg.AnnealingError, match="no couplings"):
            e.sweep_transverse(1, 2, 0.25)
        e.set_csr(*g, h)
        with pytest.raises(sg.AnnealingError, match="no replicas"):
            e.sweep_transverse(1, 2, 0.25)


def test_unsupported_problems(sg):
    from spin_glass_anneal_rl_amd import encoders as enc
    N = sg._native
    g, h = shape("lattice3")
    n = 27
    rng = np.random.RandomState(5)
    with sg.AnnealEngine(0) as e:  # dense couplings
        J = np.triu(rng.randint(0, 2, (64, 64)) * 2 - 1, 1).astype(np.float32)
        e.set_dense(J + J.T, np.zeros(64, np.float32))
        e.init_replicas(4, seed=SEED)
        e.set_temperatures(1.0)
        refused(sg, e, N.ERR_UNSUPPORTED, "dense", 1, 2, 0.25)
    with sg.AnnealEngine(0) as e:  # real-valued J: the canonical order
        e.set_csr(g[0], g[1], (g[2] * rng.uniform(0.1, 1.0, 1)[0] * np.float32(np.pi)).astype(np.float32), h)
        e.init_replicas(4, seed=SEED)
        e.set_temperatures(1.0)
        refused(sg, e, N.ERR_UNSUPPORTED, "canonical order", 1, 2, 0.25)
    with sg.AnnealEngine(0) as e:  # shared-coupling batch
        e.set_csr_shared(*g, np.zeros((2, n), np.float32))
        e.init_replicas(4, seed=SEED)
        e.set_temperatures(1.0)
        refused(sg, e, N.ERR_UNSUPPORTED, "batches", 1, 2, 0.25)
    with sg.AnnealEngine(0) as e:  # ragged batch
        small = csr_from_edges(5, [(i, i + 1, 1.0) for i in range(4)])
        e.set_csr_batch([(g[0], g[1], g[2], h), (small[0], small[1], small[2], np.zeros(5, np.float32))])
        e.init_replicas(4, seed=SEED)
        e.set_temperatures(1.0)
        refused(sg, e, N.ERR_UNSUPPORTED, "ragged", 1, 2, 0.25)
    with sg.AnnealEngine(0) as e:  # implicit group couplings
        ng, mp, mem, c, hg = gc._assignment(6, 6)
        e.set_groups(ng, (mp, mem), c, hg)
        e.init_replicas(4, seed=SEED)
        e.set_temperatures(1.0)
        refused(sg, e, N.ERR_UNSUPPORTED, "sga_set_groups", 1, 2, 0.25)
    with sg.AnnealEngine(0) as e:  # implicit TSP couplings
        xy = rng.rand(6, 2) * 100.0
        d32, A, B, ht, _ = enc.tsp_structure(np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1]), 200.0, 120.0,
                                             auto_scale=True)
        e.set_tsp(d32, A, B, ht)
        e.init_replicas(4, seed=SEED)
        e.set_temperatures(1.0)
        refused(sg, e, N.ERR_UNSUPPORTED, "sga_set_tsp", 1, 2, 0.25)
    with engine(sg, "lattice3", 4, 1.0) as e:  # another rule
        e.set_update_rule(N.RULE_GLAUBER)
        refused(sg, e, N.ERR_UNSUPPORTED, "Metropolis", 1, 2, 0.25)
        e.set_update_rule(N.RULE_METROPOLIS)
        e.sweep_transverse(1, 2, 0.25)


# ---- 11. the annealer --------------------------------------------------------------------------------------------------------------
def test_simulated_quantum_annealing_run(sg):
    g, h = shape("lattice6")
    n = 216
    J = np.zeros((n, n), np.float32)
    for i in range(n):
        J[i, g[1][g[0][i]:g[0][i + 1]]] = g[2][g[0][i]:g[0][i + 1]]
    model = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=True))
    model.set_couplings_from_matrix(torch.from_numpy(J))
    model.set_external_fields(torch.from_numpy(h))
    cfg = sg.SimulatedQuantumAnnealingConfig(n_slices=8, n_instances=2, temperature=0.05, n_sweeps=60,
                                             transverse_field=sg.TransverseField("linear_decrease", initial=3.0, final=0.05),
                                             seed=4242, measure_interval=10)
    sqa = sg.SimulatedQuantumAnnealing(cfg)
    a = sqa.run(model, measure_overlaps=True)
    b = sg.SimulatedQuantumAnnealing(cfg).run(model)
    prob = oracle.Problem(csr=g, h=h)
    spins = a.best_configuration.numpy().astype(np.int8)
    assert set(np.unique(spins)) <= {-1, 1} and a.best_energy == oracle.energy(prob, spins)
    assert a.best_energy == b.best_energy and torch.equal(a.best_configuration, b.best_configuration)
    assert a.energy_history == b.energy_history and len(a.energy_history) == 6
    assert a.best_energy <= min(a.energy_history)
    assert a.algorithm == "simulated_quantum_annealing" and a.n_sweeps == 60
    assert sqa.final_energies.shape == (2, 8) and sqa.slice_overlaps.shape == (16, 16)
    assert np.all(np.diag(sqa.slice_overlaps) == n)
    # the upstream README's call
    base = sg.GPUAnnealer(sg.GPUAnnealerConfig(n_sweeps=30, final_temp=0.05, random_seed=7, record_interval=10))
    q = sg.QuantumFluctuations(base_annealer=base, transverse_field_schedule="linear_decrease", initial_field_strength=3.0)
    r1 = q.simulated_quantum_anneal(model, n_trotter_slices=4, quantum_monte_carlo=True)
    r2 = q.path_integral_mc(model, imaginary_time_slices=6, quantum_temperature=0.1)
    for r in (r1, r2):
        assert r.best_energy == oracle.energy(prob, r.best_configuration.numpy().astype(np.int8))
    # no classical fallback: a dense model is refused with the engine's reason
    dense = sg.IsingModel(sg.IsingModelConfig(n_spins=64, use_sparse=False))
    Jd = torch.triu((torch.randint(0, 2, (64, 64)) * 2 - 1).float(), 1)
    dense.set_couplings_from_matrix(Jd + Jd.T)
    with pytest.raises(sg.AnnealingError, match="dense"):
        q.simulated_quantum_anneal(dense, n_trotter_slices=4)
