"""World-line cluster updates on the device (sga_worldline_clusters, csrc/worldline_clusters.hip) against the plain-Python
specification of tests/worldline_reference.py: spins, energies, bests and the segment counts bit for bit (np.array_equal),
on the shapes of test_transverse_gpu.py -- 3^3 and 6^3 periodic +-J lattices and a random graph of 300 sites (degree ~8,
|J| <= 5, half-integer h, one empty row) -- with (P, G) in {(2, 3), (3, 1), (4, 3), (32, 1), (34, 1), (64, 1)}: both word
widths of the spins in LDS, an odd P and the first P past 32.  A distinct p_bond per sweep and group; 3 sweeps, 1 at
P >= 32 (the reference costs one oracle call per lane and site).  A reference is computed once per case and shared."""
import functools

import numpy as np
import pytest
import torch

import groups_cases as gc
import oracle
import worldline_reference as wr
from test_cluster_moves_gpu import SEED, csr_from_edges, state
from test_transverse_gpu import SHAPES, engine, shape, temps

pytestmark = pytest.mark.gpu

PG = [(2, 3), (3, 1), (4, 3), (32, 1), (34, 1), (64, 1)]
ROUND = 0xFFFFFFFE  # round + kk wraps through 2^32 within a call of 3 sweeps


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def sweeps_of(P):
    return 1 if P >= 32 else 3


def bonds(ns, G):
    """A different p_bond per sweep and per group, out of {0.3, 0.85, 0.6, 1 - 2^-20}."""
    vals = np.asarray([0.3, 0.85, 0.6, 1.0 - 2.0 ** -20])
    return vals[(np.arange(ns)[:, None] + 2 * np.arange(G)[None, :]) % 4]


def problem(name):
    g, h = shape(name)
    return oracle.Problem(csr=g, h=h)


@functools.lru_cache(maxsize=None)
def reference(name, P, G):
    """(spins, out) of sweeps_of(P) sweeps from the engine's initial replicas; read only."""
    prob = problem(name)
    S = oracle.init_spins(prob.n, P * G, SEED)
    out = wr.sweeps(prob, S, temps(P, G), sweeps_of(P), P, bonds(sweeps_of(P), G), seed=SEED, round=ROUND)
    return S, out


def assert_matches(e, S, out, stats=None):
    st = state(e)
    assert np.array_equal(st["S"], S)
    assert np.array_equal(st["E"], out["energy"])
    assert np.array_equal(st["be"], out["best_energy"])
    assert np.array_equal(st["bs"], out["best_spins"])
    assert not st["acc"].any()  # the accept counters are the sweeps' own
    if stats is not None:
        assert stats.dtype == np.int64 and np.array_equal(stats, out["stats"])


def assert_same_state(a, b):
    for key in ("S", "E", "acc", "be", "bs"):
        assert np.array_equal(a[key], b[key]), key


# ---- 1. against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,G", PG)
@pytest.mark.parametrize("name", SHAPES)
def test_against_the_reference(sg, name, P, G):
    S, out = reference(name, P, G)
    ns = sweeps_of(P)
    with engine(sg, name, P * G, temps(P, G)) as e:
        stats = e.worldline_clusters(ns, P, bonds(ns, G), round=ROUND, stats=True)
        assert_matches(e, S, out, stats)
        n = S.shape[1]
        assert np.all(stats[:, 0] < ns * n * P) and np.all(stats[:, 1] > 0) and np.all(stats[:, 2] > stats[:, 1])
        assert ("64-bit" if P > 32 else "32-bit") in e.last_kernel() and "worldline_clusters_kernel" in e.last_kernel()
        # the tracked energies are the classical ones
        E = e.energies()
        e.recompute_energies()
        assert np.array_equal(e.energies(), E)
        assert np.array_equal(E, [oracle.energy(problem(name), r) for r in S])


# ---- 2. the limits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,P,G", [("lattice3", 2, 3), ("lattice6", 3, 1), ("random300", 4, 3)])
def test_no_bonds_is_the_single_spin_rule(sg, name, P, G):
    """p_bond = 0: every slice walks the sites in typewriter order under the oracle's fp64 Metropolis update with its own
    uniform."""
    prob = problem(name)
    T = temps(P, G)
    S = oracle.init_spins(prob.n, P * G, SEED)
    E = np.asarray([oracle.energy(prob, s) for s in S])
    for r in range(P * G):
        for kk in range(2):
            for i in range(prob.n):
                E[r] += oracle.metropolis_update(prob, S[r], i, T[r], float(wr.draws(SEED, i, 9 + kk, r)[1]))[1]
    with engine(sg, name, P * G, T) as e:
        stats = e.worldline_clusters(2, P, 0.0, round=9, stats=True)
        assert np.array_equal(e.spins(), S) and np.array_equal(e.energies(), E)
        assert np.all(stats[:, 0] == 2 * prob.n * P) and np.array_equal(stats[:, 1], stats[:, 2])


@pytest.mark.parametrize("name", ["lattice6", "random300"])
def test_all_bonds_on_identical_slices(sg, name):
    """p_bond = 1 and identical slices, P = 4, T = 2: the slices stay identical and walk as one replica at T / P = 0.5 under
    slice 0's uniforms."""
    prob = problem(name)
    P, G, T, n = 4, 2, 2.0, problem(name).n
    one = oracle.init_spins(n, G, SEED)
    s0 = np.repeat(one, P, axis=0)
    E, flips = np.asarray([oracle.energy(prob, s) for s in one]), np.zeros(G, np.int64)
    for g in range(G):
        for kk in range(2):
            for i in range(n):
                took, dE = oracle.metropolis_update(prob, one[g], i, T / P, float(wr.draws(SEED, i, 3 + kk, g * P)[1]))
                E[g] += dE
                flips[g] += took
    with engine(sg, name, P * G, T, s0=s0) as e:
        stats = e.worldline_clusters(2, P, 1.0, round=3, stats=True)
        assert np.array_equal(e.spins(), np.repeat(one, P, axis=0))
        assert np.array_equal(e.energies(), np.repeat(E, P))
        assert np.array_equal(stats, np.stack([np.full(G, 2 * n), flips, P * flips], axis=1)) and np.all(flips > 0)


@pytest.mark.parametrize("name,P", [("lattice6", 4), ("random300", 3)])
def test_temperature_limits(sg, name, P):
    G, ns = 3, 2
    prob = problem(name)
    T = np.repeat([0.0, np.inf, 1.0], P)
    S = oracle.init_spins(prob.n, P * G, SEED)
    out = wr.sweeps(prob, S, T, ns, P, bonds(ns, G), seed=SEED, round=1)
    with engine(sg, name, P * G, T) as e:
        stats = e.worldline_clusters(ns, P, bonds(ns, G), round=1, stats=True)
        assert_matches(e, S, out, stats)
    assert stats[1, 0] == stats[1, 1]  # T = inf flips every segment
    assert 0 < stats[0, 1] < stats[0, 0]  # T = 0 flips the segments that do not raise the energy, summed over their slices


# ---- 3. independence of call shape and sharding ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,P,G", [("lattice3", 2, 3), ("lattice6", 4, 3), ("random300", 34, 1)])
def test_two_sweeps_are_two_calls(sg, name, P, G):
    b = bonds(2, G)
    T = temps(P, G)
    with engine(sg, name, P * G, T) as e, engine(sg, name, P * G, T) as twin:
        sa = e.worldline_clusters(2, P, b, round=0xFFFFFFFF, stats=True)
        sb = twin.worldline_clusters(1, P, b[:1], round=0xFFFFFFFF, stats=True)
        sb += twin.worldline_clusters(1, P, b[1:], round=0, stats=True)  # (round + 1 wraps)
        assert_same_state(state(e), state(twin))
        assert np.array_equal(sa, sb)


@pytest.mark.parametrize("name,P", [("lattice3", 2), ("lattice6", 3), ("random300", 4)])
def test_sharded_groups(sg, name, P):
    G, ns = 3, 2
    b = bonds(ns, G)
    T = temps(P, G)
    with engine(sg, name, P * G, T) as full:
        all_stats = full.worldline_clusters(ns, P, b, round=4, stats=True)
        want = state(full)
    for g0, gn in ((1, 2), (2, 1)):  # the last two groups, the last one
        lo, R = g0 * P, gn * P
        with engine(sg, name, R, T[lo:], R_global=P * G, replica0=lo) as part:
            stats = part.worldline_clusters(ns, P, b[:, g0:], round=4, stats=True)
            got = state(part)
            for key in ("S", "E", "acc", "be", "bs"):
                assert np.array_equal(got[key], want[key][lo:lo + R]), key
            assert np.array_equal(stats, all_stats[g0:])


# ---- 4. what moves and what does not ----------------------------------------------------------------------------------------------
def test_counters_ladder_and_exchange_statistics(sg):
    name, P, G = "lattice6", 4, 3
    with engine(sg, name, P * G, 1.0) as e, engine(sg, name, P * G, 1.0) as twin:
        for x in (e, twin):
            x.set_ladder(np.tile([0.5, 1.0, 2.0, 4.0], G), n_ladders=G)
            x.sweep(2)
            x.exchange()
            x.exchange()
        slot, xstats, T, (acc, att) = e.slot_map(), e.exchange_stats(), e.temperatures(), e.stats()
        assert xstats[0].sum() > 0 and e.counters() == (2, 2)
        before = e.spins()
        assert e.worldline_clusters(2, P, 0.5) is None  # round = sweeps_done = 2
        assert not np.array_equal(e.spins(), before)
        assert e.counters() == (2, 2)
        assert np.array_equal(e.slot_map(), slot) and np.array_equal(e.temperatures(), T)
        assert all(np.array_equal(a, b) for a, b in zip(e.exchange_stats(), xstats))
        assert np.array_equal(e.stats()[0], acc) and np.array_equal(e.stats()[1], att)
        assert "worldline_clusters_kernel" in e.last_kernel()
        twin.worldline_clusters(2, P, 0.5, round=2)
        assert_same_state(state(e), state(twin))
        mid = state(e)
        stats = np.full((G, 3), 5, np.int64)
        e.worldline_clusters(0, P, 0.5)  # a no-op
        N = sg._native
        b = np.zeros((0, G))
        assert N.lib().sga_worldline_clusters(e._h, 0, P, 0, b.ctypes.data, stats.ctypes.data) == N.OK
        assert_same_state(state(e), mid)
        assert np.all(stats == 5)
        # stats are added to the caller's array
        one = np.full((1, G), 0.5)
        assert N.lib().sga_worldline_clusters(e._h, 1, P, 7, one.ctypes.data, stats.ctypes.data) == N.OK
        assert np.array_equal(stats - 5, twin.worldline_clusters(1, P, 0.5, round=7, stats=True))


@pytest.mark.parametrize("name", ["lattice3", "lattice6"])
def test_field_cache_is_reseeded(sg, name):
    P, G = 4, 3
    T = temps(P, G)
    with engine(sg, name, P * G, T, cache="on") as e, engine(sg, name, P * G, T, cache="on") as twin:
        e.sweep(1)
        twin.sweep(1)
        assert "sweep_clf_csr_kernel" in e.last_kernel()  # the fields are resident and valid now
        e.worldline_clusters(2, P, bonds(2, G))
        mid = state(e)
        for r in range(P * G):
            twin.set_spins(r, mid["S"][r])
        assert np.array_equal(twin.energies(), mid["E"]) and e.counters() == twin.counters()
        e.sweep(2)
        twin.sweep(2)
        assert "sweep_clf_csr_kernel" in e.last_kernel()
        a, b = state(e), state(twin)
        assert np.array_equal(a["S"], b["S"]) and np.array_equal(a["E"], b["E"])
        e.recompute_energies()
        assert np.array_equal(e.energies(), a["E"])


# ---- 5. refusals leave the engine as it was ----------------------------------------------------------------------------------------
def refused(sg, e, code, word, *args, **kw):
    ragged = getattr(e, "_sizes", None) is not None  # (best(r) of a ragged batch has the model's own length)
    before = dict(S=e.spins(), E=e.energies(), acc=e.stats()[0]) if ragged else state(e)
    counters = e.counters()
    with pytest.raises(sg.AnnealingError) as err:
        e.worldline_clusters(*args, **kw)
    assert err.value.details["code"] == code and word in str(err.value), str(err.value)
    now = dict(S=e.spins(), E=e.energies(), acc=e.stats()[0]) if ragged else state(e)
    assert all(np.array_equal(now[key], before[key]) for key in before)
    assert e.counters() == counters


def test_invalid_calls(sg):
    N = sg._native
    with engine(sg, "lattice3", 12, 1.0) as e:
        e.sweep(1)
        for P in (1, 0, -2, 5, 8, 24, 65):
            refused(sg, e, N.ERR_INVALID, "n_slices", 1, P, 0.25)
        refused(sg, e, N.ERR_INVALID, "n_sweeps", -1, 4, 0.25)
        for bad in (np.nan, np.inf, -1e-9, 1.0 + 1e-12, [[0.25, 0.25, np.nan]]):
            refused(sg, e, N.ERR_INVALID, "p_bond", 1, 4, bad)
        assert N.lib().sga_worldline_clusters(e._h, 1, 4, 0, None, None) == N.ERR_INVALID
        b = np.zeros(3, np.float64)
        assert N.lib().sga_worldline_clusters(None, 1, 4, 0, b.ctypes.data, None) == N.ERR_INVALID
        dev = torch.zeros(3, dtype=torch.float64, device="cuda")
        assert N.lib().sga_worldline_clusters(e._h, 1, 4, 0, dev.data_ptr(), None) == N.ERR_INVALID
        dev_stats = torch.zeros(9, dtype=torch.int64, device="cuda")
        assert N.lib().sga_worldline_clusters(e._h, 1, 4, 0, b.ctypes.data, dev_stats.data_ptr()) == N.ERR_INVALID
        assert e.counters() == (1, 0)
        e.worldline_clusters(1, 3, 0.25)  # an odd P is served
    with engine(sg, "lattice3", 8, 1.0, R_global=16, replica0=6) as e:  # replica0 % 4 != 0
        refused(sg, e, N.ERR_INVALID, "replica0", 1, 4, 0.25)
        e.worldline_clusters(1, 2, 0.25)  # 6 % 2 == 0
    g, h = shape("lattice3")
    with sg.AnnealEngine(0) as e:
        with pytest.raises(sg.AnnealingError, match="no couplings"):
            e.worldline_clusters(1, 2, 0.25)
        e.set_csr(*g, h)
        with pytest.raises(sg.AnnealingError, match="no replicas"):
            e.worldline_clusters(1, 2, 0.25)


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
    with sg.AnnealEngine(0) as e:  # a group's spin words beyond LDS: a chain of 41 000 sites, 4 slices
        m = 41000
        chain = (np.concatenate([[0], np.cumsum(np.r_[1, np.full(m - 2, 2), 1])]).astype(np.int32),
                 np.asarray([j for i in range(m) for j in (i - 1, i + 1) if 0 <= j < m], np.int32), np.ones(2 * (m - 1), np.float32))
        e.set_csr(*chain, np.zeros(m, np.float32))
        e.init_replicas(4, seed=SEED)
        e.set_temperatures(1.0)
        with pytest.raises(sg.AnnealingError, match="spin words do not fit LDS") as err:
            e.worldline_clusters(1, 4, 0.25)
        assert err.value.details["code"] == N.ERR_UNSUPPORTED
        e.sweep_transverse(1, 4, 0.25)  # (the transverse sweep serves it)
    with engine(sg, "lattice3", 4, 1.0) as e, engine(sg, "lattice3", 4, 1.0) as twin:  # another rule: the call brings its own
        e.set_update_rule(N.RULE_GLAUBER)
        e.worldline_clusters(1, 2, 0.25, round=0)
        twin.worldline_clusters(1, 2, 0.25, round=0)
        assert_same_state(state(e), state(twin))


# ---- 6. the annealer -----------------------------------------------------------------------------------------------------------------
def lattice6_model(sg):
    g, h = shape("lattice6")
    n = 216
    J = np.zeros((n, n), np.float32)
    for i in range(n):
        J[i, g[1][g[0][i]:g[0][i + 1]]] = g[2][g[0][i]:g[0][i + 1]]
    model = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=True))
    model.set_couplings_from_matrix(torch.from_numpy(J))
    model.set_external_fields(torch.from_numpy(h))
    return model


def test_simulated_quantum_annealing_with_clusters(sg):
    model, prob = lattice6_model(sg), problem("lattice6")
    tf = sg.TransverseField("linear_decrease", initial=3.0, final=0.05)
    cfg = sg.SimulatedQuantumAnnealingConfig(n_slices=8, n_instances=2, temperature=0.05, n_sweeps=60, transverse_field=tf, seed=4242,
                                             measure_interval=10, worldline_clusters=True, cluster_interval=3)
    sqa = sg.SimulatedQuantumAnnealing(cfg)
    a = sqa.run(model)
    other = sg.SimulatedQuantumAnnealing(cfg)
    b = other.run(model)
    spins = a.best_configuration.numpy().astype(np.int8)
    assert set(np.unique(spins)) <= {-1, 1} and a.best_energy == oracle.energy(prob, spins)
    assert a.best_energy == b.best_energy and torch.equal(a.best_configuration, b.best_configuration)
    assert a.energy_history == b.energy_history and len(a.energy_history) == 6
    assert a.best_energy <= min(a.energy_history)
    st = sqa.cluster_statistics
    assert st.shape == (3,) and st.dtype == np.int64 and np.array_equal(st, other.cluster_statistics)
    assert 20 * 216 * 2 <= st[0] <= 20 * 216 * 16 and 0 < st[1] <= st[0] and st[2] >= st[1]  # 20 cluster sweeps, 2 groups of 8
    # the flag of run() overrides the configuration's; off is the transverse sweeps alone
    plain = sg.SimulatedQuantumAnnealingConfig(n_slices=8, n_instances=2, temperature=0.05, n_sweeps=60, transverse_field=tf, seed=4242,
                                               measure_interval=10)
    off = sg.SimulatedQuantumAnnealing(plain)
    c = off.run(model)
    assert off.cluster_statistics is None
    d = sg.SimulatedQuantumAnnealing(cfg).run(model, worldline_clusters=False)
    on = sg.SimulatedQuantumAnnealing(plain)
    f = on.run(model, worldline_clusters=True)
    assert np.array_equal(on.cluster_statistics[:1] > 0, [True])
    assert c.energy_history == d.energy_history and torch.equal(c.best_configuration, d.best_configuration)
    assert f.energy_history != c.energy_history
    # ... and equals the run as it was before the flag existed: the engine driven by hand
    k = plain.couplings()
    history = []
    with sg.AnnealEngine(0) as eng:
        model.load_into(eng)
        eng.init_replicas(16, seed=4242)
        eng.set_temperatures(8 * 0.05)
        for k0 in range(0, 60, 10):
            eng.sweep_transverse(10, 8, k[k0:k0 + 10])
            history.append(float(eng.energies().min()))
        best_energy, best_spins, _ = eng.best()
    assert c.energy_history == history and c.best_energy == float(best_energy)
    assert np.array_equal(c.best_configuration.numpy().astype(np.int8), best_spins)
    # the upstream entry point passes the keyword through
    base = sg.GPUAnnealer(sg.GPUAnnealerConfig(n_sweeps=30, final_temp=0.05, random_seed=7, record_interval=10))
    q = sg.QuantumFluctuations(base_annealer=base, transverse_field_schedule="linear_decrease", initial_field_strength=3.0,
                               worldline_clusters=True)
    r = q.simulated_quantum_anneal(model, n_trotter_slices=4)
    assert r.best_energy == oracle.energy(prob, r.best_configuration.numpy().astype(np.int8))
    assert q.last.cluster_statistics[0] >= 30 * 216
