"""World-line cluster updates on dense couplings on the device (sga_worldline_clusters_dense,
csrc/worldline_clusters_dense.hip) against the plain-Python specification of tests/worldline_reference.py run on the same
couplings as full CSR rows: spins, energies, bests and statistics bit for bit (np.array_equal) on the cases of
tests/worldline_dense_cases.py -- n = 24 (shorter than a block), 130 (several blocks, a tail of 2 sites, padded rows), 300
(int32 fields), 1100 (several row chunks per wave, 34 blocks and a tail); 2 <= P <= 64, odd P included; h zero, integer and
half-integer; int8 and fp32 rows; an independent and a correlated start.  The reference runs are computed once per case
and shared.  test_fields_stay_valid is the one that a kernel with right decisions and a wrong field update cannot pass."""
import numpy as np
import pytest
import torch

import groups_cases as gc
import oracle
import transverse_dense_cases as dc
import transverse_reference as tr
import worldline_dense_cases as wc
import worldline_reference as wr
from test_cluster_moves_gpu import state
from test_transverse_dense_gpu import assert_same_state, engine

pytestmark = pytest.mark.gpu

NS, SEED = wc.NS, wc.SEED
STORAGES = ["i8", "f32"]
KEYS = ("S", "E", "acc", "be", "bs")
KERNEL = "worldline_clusters_dense_kernel"


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def assert_matches(e, S, out):
    st = state(e)
    assert np.array_equal(st["S"], S)
    assert np.array_equal(st["E"], out["energy"])
    assert np.array_equal(st["be"], out["best_energy"])
    assert np.array_equal(st["bs"], out["best_spins"])
    assert not st["acc"].any()


# ---- 1. against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("start", wc.STARTS)
@pytest.mark.parametrize("kind", wc.H_KINDS)
@pytest.mark.parametrize("n,P,G", wc.GRID)
def test_against_the_reference(sg, n, P, G, kind, start, storage):
    S0, S, out = wc.reference(n, kind, P, G, start)
    wc.check_counts(out, start)
    with engine(sg, n, kind, P * G, dc.temps(n, P, G), storage, seed=SEED, s0=S0) as e:
        assert np.array_equal(e.energies(), out["energy0"])
        stats = e.worldline_clusters_dense(NS, P, wc.p_bond(start, G), round=wc.round0(start), stats=True)
        lk = e.last_kernel()
        assert KERNEL in lk and ("int8_t" if storage == "i8" else "float") in lk, lk
        assert ("int32_t" if n == 300 else "int16_t") in lk and "%d slices" % P in lk, lk
        assert_matches(e, S, out)
        assert np.array_equal(stats, out["stats"])
        assert e.counters() == (0, 0) and not e.stats()[1].any()
        E = e.energies()
        e.recompute_energies()
        assert np.array_equal(e.energies(), E)


# ---- 2. limits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("n,kind,P", [(130, "half", 4), (24, "int", 3)])
def test_no_bonds_is_the_single_spin_rule(sg, n, kind, P, storage):
    """p_bond = 0: every slice walks the typewriter Metropolis chain of the oracle under its own uniforms."""
    prob, T = dc.problem(n, kind), dc.SHAPE[n]["T0"]
    S = oracle.init_spins(n, P, SEED)
    E = np.asarray([oracle.energy(prob, r) for r in S])
    flips = 0
    for kk in range(NS):
        for p in range(P):
            for i in range(n):
                took, dE = oracle.metropolis_update(prob, S[p], i, T, float(wr.draws(SEED, i, 7 + kk, p)[1]), arith=oracle.ARITH_F64)
                E[p] += dE
                flips += took
    with engine(sg, n, kind, P, T, storage, seed=SEED) as e:
        stats = e.worldline_clusters_dense(NS, P, 0.0, round=7, stats=True)
        assert np.array_equal(e.spins(), S) and np.array_equal(e.energies(), E)
        assert np.array_equal(stats, [[NS * n * P, flips, flips]]) and 0 < flips < NS * n * P


@pytest.mark.parametrize("storage", STORAGES)
def test_all_bonds_on_identical_slices_is_one_replica_at_T_over_P(sg, storage):
    """p_bond = 1 on identical slices, P = 4, T = 8: the slices stay identical and walk the one-replica typewriter chain at
    T / P = 2 under slice 0's uniforms (powers of two keep -P dE / T exact)."""
    n, kind, P, T = 130, "half", 4, 8.0
    prob = dc.problem(n, kind)
    one = oracle.init_spins(n, 1, SEED)[0]
    s0 = np.repeat(one[None, :], P, axis=0).copy()
    E, flips = oracle.energy(prob, one), 0
    for kk in range(NS):
        for i in range(n):
            took, dE = oracle.metropolis_update(prob, one, i, T / P, float(wr.draws(SEED, i, 5 + kk, 0)[1]))
            E += dE
            flips += took
    with engine(sg, n, kind, P, T, storage, seed=SEED, s0=s0) as e:
        stats = e.worldline_clusters_dense(NS, P, 1.0, round=5, stats=True)
        assert all(np.array_equal(r, one) for r in e.spins())
        assert np.array_equal(e.energies(), np.full(P, E))
        assert np.array_equal(stats, [[NS * n, flips, P * flips]]) and 0 < flips < NS * n


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("n,P", [(130, 4), (24, 3)])
def test_temperature_limits(sg, n, P, storage):
    G, kind = 3, "half"
    T = np.repeat([0.0, np.inf, dc.SHAPE[n]["T0"]], P)
    S = oracle.init_spins(n, P * G, SEED)
    out = wr.sweeps(dc.problem(n, kind, as_csr=True), S, T, NS, P, 0.6, seed=SEED, round=2)
    assert out["stats"][1, 0] == out["stats"][1, 1] and out["stats"][0, 1] < out["stats"][0, 0]  # T = inf flips every segment
    with engine(sg, n, kind, P * G, T, storage, seed=SEED) as e:
        stats = e.worldline_clusters_dense(NS, P, 0.6, round=2, stats=True)
        assert_matches(e, S, out)
        assert np.array_equal(stats, out["stats"])


# ---- 3. composition --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,P,G,storage", [(24, 3, 1, "i8"), (130, 4, 3, "f32"), (300, 2, 1, "i8"), (1100, 4, 1, "f32")])
def test_two_sweeps_are_two_calls_across_the_wrap(sg, n, P, G, storage):
    S0, S, out = wc.reference(n, "half", P, G, "correlated")
    T, b = dc.temps(n, P, G), wc.p_bond("correlated", G)
    with engine(sg, n, "half", P * G, T, storage, seed=SEED, s0=S0) as e, engine(sg, n, "half", P * G, T, storage, seed=SEED, s0=S0) as twin:
        sa = e.worldline_clusters_dense(2, P, b, round=wc.WRAP_ROUND, stats=True)
        sb = twin.worldline_clusters_dense(1, P, b[:1], round=wc.WRAP_ROUND, stats=True)
        sb += twin.worldline_clusters_dense(1, P, b[1:], round=0, stats=True)
        assert_same_state(state(e), state(twin))
        assert np.array_equal(sa, sb) and np.array_equal(sa, out["stats"])
        assert_matches(e, S, out)


@pytest.mark.parametrize("n,P,storage", [(24, 2, "f32"), (130, 4, "i8")])
def test_sharded_groups(sg, n, P, storage):
    G = 3
    T, b = dc.temps(n, P, G), wc.p_bond("independent", G)
    S0, S, out = wc.reference(n, "int", P, G, "independent")
    with engine(sg, n, "int", P * G, T, storage, seed=SEED) as full:
        all_stats = full.worldline_clusters_dense(NS, P, b, round=0, stats=True)
        want = state(full)
        assert np.array_equal(want["S"], S)
    for g0, gn in ((1, 2), (2, 1)):  # the last two groups, the last one
        lo, R = g0 * P, gn * P
        with engine(sg, n, "int", R, T[lo:], storage, seed=SEED, R_global=P * G, replica0=lo) as part:
            stats = part.worldline_clusters_dense(NS, P, b[:, g0:], round=0, stats=True)
            got = state(part)
            for key in KEYS:
                assert np.array_equal(got[key], want[key][lo:lo + R]), key
            assert np.array_equal(stats, all_stats[g0:])


# ---- 4. the same integer couplings held as CSR under sga_worldline_clusters --------------------------------------------------------------
@pytest.mark.parametrize("start", wc.STARTS)
@pytest.mark.parametrize("kind,P,G", [("int", 4, 3), ("half", 34, 1)])
def test_csr_engine_walks_the_same_chain(sg, kind, P, G, start):
    n = 130
    T, b, S0 = dc.temps(n, P, G), wc.p_bond(start, G), wc.start_spins(start, n, P, G)
    with engine(sg, n, kind, P * G, T, "f32", seed=SEED, s0=S0) as e, sg.AnnealEngine(0) as c:
        c.set_csr(*dc.csr(n), dc.fields(n, kind))
        c.init_replicas(P * G, seed=SEED, s0=S0)
        c.set_temperatures(T)
        se = e.worldline_clusters_dense(NS, P, b, round=wc.round0(start), stats=True)
        sc = c.worldline_clusters(NS, P, b, round=wc.round0(start), stats=True)
        assert "worldline_clusters_kernel" in c.last_kernel() and KERNEL in e.last_kernel()
        assert_same_state(state(e), state(c))
        assert np.array_equal(se, sc) and se[:, 1].all()


# ---- 5. the fields stay valid ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("n,kind", [(130, "half"), (300, "int")])
def test_fields_stay_valid(sg, n, kind, storage):
    """sweep(1) cached, the cluster call, sweep_transverse_dense(2), sweep(2): the sweeps after the call go on from the
    fields the call updated -- against a twin that is given the spins by set_spins and seeds its fields from them."""
    P, G = 4, 3 if n == 130 else 1
    T = dc.temps(n, P, G)
    with engine(sg, n, kind, P * G, T, storage) as e, engine(sg, n, kind, P * G, T, storage) as twin:
        e.sweep(1)
        assert "sweep_clf" in e.last_kernel()  # the fields are resident and valid now
        stats = e.worldline_clusters_dense(2, P, 0.6, round=11, stats=True)
        assert KERNEL in e.last_kernel() and stats[:, 2].min() > n // 4  # flips in every block
        mid = state(e)
        for r in range(P * G):
            twin.set_spins(r, mid["S"][r])
        twin.set_counters(*e.counters())
        assert np.array_equal(twin.energies(), mid["E"])
        for step in (lambda x: x.sweep_transverse_dense(2, P, dc.k_perp(G)[:2]), lambda x: x.sweep(2)):
            step(e)
            step(twin)
            a, b = state(e), state(twin)
            assert np.array_equal(a["S"], b["S"]) and np.array_equal(a["E"], b["E"])
        assert "sweep_clf" in e.last_kernel()
        E = e.energies()
        e.recompute_energies()
        assert np.array_equal(e.energies(), E)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("n,kind,P,G", [(130, "half", 4, 3), (300, "int", 2, 1)])
def test_sweeps_and_clusters_in_turn(sg, n, kind, P, G, storage):
    """Three rounds of (dense transverse sweep, cluster sweep) against the two references chained, energies and bests handed
    on: neither call seeds the fields after the first."""
    T = dc.temps(n, P, G)
    dense, sparse = dc.problem(n, kind), dc.problem(n, kind, as_csr=True)
    bonds = wc.P_CYCLE[[0, 3, 2]]
    S = oracle.init_spins(n, P * G, SEED)
    rec = dict(energy=None, best_energy=None, best_spins=None)
    acc, want = np.zeros(P * G, np.int64), np.zeros((G, 3), np.int64)
    for t in range(3):  # (the cluster sweep after transverse sweep t draws at the engine's sweeps_done, t + 1)
        got = tr.sweeps(dense, S, T, 1, P, dc.k_perp(G)[t:t + 1], seed=SEED, sweep0=t, **rec)
        acc += got["n_accepted"]
        rec = {key: got[key] for key in rec}
        got = wr.sweeps(sparse, S, T, 1, P, bonds[t], seed=SEED, round=t + 1, **rec)
        want += got["stats"]
        rec = {key: got[key] for key in rec}
    with engine(sg, n, kind, P * G, T, storage, seed=SEED) as e:
        have = np.zeros((G, 3), np.int64)
        for t in range(3):
            e.sweep_transverse_dense(1, P, dc.k_perp(G)[t:t + 1])
            have += e.worldline_clusters_dense(1, P, bonds[t], stats=True)
        assert e.counters() == (3, 0)
        st = state(e)
        assert np.array_equal(st["S"], S) and np.array_equal(st["E"], rec["energy"])
        assert np.array_equal(st["be"], rec["best_energy"]) and np.array_equal(st["bs"], rec["best_spins"])
        assert np.array_equal(st["acc"], acc) and np.array_equal(have, want) and have[:, 2].all()


# ---- 6. seeding ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", ["off", "auto"])
@pytest.mark.parametrize("storage", STORAGES)
def test_the_call_seeds_the_fields_after_an_uncached_sweep(sg, storage, cache):
    n, kind, P, G = 130, "half", 4, 3
    T = dc.temps(n, P, G)
    with engine(sg, n, kind, P * G, T, storage, cache=cache) as e, engine(sg, n, kind, P * G, T, storage, cache="on") as twin:
        for rnd in (3, 4):
            e.sweep(1)  # (cache off: the row kernels move the spins only)
            twin.sweep(1)
            assert ("sweep_clf" not in e.last_kernel() or cache == "auto") and "sweep_clf" in twin.last_kernel()
            sa = e.worldline_clusters_dense(1, P, 0.6, round=rnd, stats=True)
            sb = twin.worldline_clusters_dense(1, P, 0.6, round=rnd, stats=True)
            assert_same_state(state(e), state(twin))
            assert np.array_equal(sa, sb) and sa[:, 2].all()


# ---- 7. what must not move ---------------------------------------------------------------------------------------------------------------------
def test_counters_ladder_and_exchange_statistics(sg):
    n, P, G = 130, 4, 3
    with engine(sg, n, "int", P * G, 1.0) as e:
        e.set_ladder(np.tile(np.asarray([0.5, 1.0, 2.0, 4.0]) * dc.SHAPE[n]["T0"], G), n_ladders=G)
        e.sweep(2)
        e.exchange()
        e.exchange()
        slot, xs, T = e.slot_map(), e.exchange_stats(), e.temperatures()
        acc, att = e.stats()
        assert xs[0].sum() > 0 and e.counters() == (2, 2)
        stats = e.worldline_clusters_dense(NS, P, 0.6, stats=True)
        assert stats[:, 2].all() and KERNEL in e.last_kernel()
        assert e.counters() == (2, 2)
        assert np.array_equal(e.slot_map(), slot) and np.array_equal(e.temperatures(), T)
        assert all(np.array_equal(a, b) for a, b in zip(e.exchange_stats(), xs))
        assert np.array_equal(e.stats()[0], acc) and np.array_equal(e.stats()[1], att)
        before = state(e)
        assert e.worldline_clusters_dense(0, P, 0.6, stats=True).sum() == 0  # a no-op
        assert_same_state(before, state(e))


# ---- 8. refusals leave the engine as it was ------------------------------------------------------------------------------------------------------
def refused(sg, e, code, word, *args, **kw):
    ragged = getattr(e, "_sizes", None) is not None  # (best(r) of a ragged batch has the model's own length)
    before = dict(S=e.spins(), E=e.energies(), acc=e.stats()[0]) if ragged else state(e)
    counters = e.counters()
    with pytest.raises(sg.AnnealingError) as err:
        e.worldline_clusters_dense(*args, **kw)
    assert err.value.details["code"] == code and word in str(err.value), str(err.value)
    now = dict(S=e.spins(), E=e.energies(), acc=e.stats()[0]) if ragged else state(e)
    assert all(np.array_equal(now[key], before[key]) for key in before)
    assert e.counters() == counters


def test_invalid_calls(sg):
    N = sg._native
    n = 24
    with engine(sg, n, "int", 12, 4.0) as e:
        e.sweep(1)
        for P in (1, 0, -2, 5, 8, 24):
            refused(sg, e, N.ERR_INVALID, "n_slices", 1, P, 0.5)
        refused(sg, e, N.ERR_INVALID, "n_sweeps", -1, 4, 0.5)
        for bad in (np.nan, 1.5, -0.1, np.inf, [[0.5, 0.5, np.nan]]):
            refused(sg, e, N.ERR_INVALID, "p_bond", 1, 4, bad)
        b = np.full(3, 0.5)
        fn = N.lib().sga_worldline_clusters_dense
        assert fn(e._h, 1, 4, 0, None, None) == N.ERR_INVALID
        assert fn(None, 1, 4, 0, b.ctypes.data, None) == N.ERR_INVALID
        dev = torch.zeros(9, dtype=torch.float64, device="cuda")
        assert fn(e._h, 1, 4, 0, dev.data_ptr(), None) == N.ERR_INVALID
        assert fn(e._h, 1, 4, 0, b.ctypes.data, dev.data_ptr()) == N.ERR_INVALID
        assert e.counters() == (1, 0)
        e.worldline_clusters_dense(1, 3, 0.5)  # an odd P is served
    with engine(sg, n, "int", 130, 4.0) as e:
        refused(sg, e, N.ERR_INVALID, "at most 64", 1, 65, 0.5)
    with engine(sg, n, "int", 8, 4.0, R_global=16, replica0=6) as e:  # replica0 % 4 != 0
        refused(sg, e, N.ERR_INVALID, "replica0", 1, 4, 0.5)
        e.worldline_clusters_dense(1, 2, 0.5)  # 6 % 2 == 0
    with sg.AnnealEngine(0) as e:
        with pytest.raises(sg.AnnealingError, match="no couplings"):
            e.worldline_clusters_dense(1, 2, 0.5)
        e.set_dense(dc.couplings(n), dc.fields(n, "int"))
        with pytest.raises(sg.AnnealingError, match="no replicas"):
            e.worldline_clusters_dense(1, 2, 0.5)
    with sg.AnnealEngine(0) as e:  # an argument error comes before the problem's kind
        e.set_csr(*dc.csr(n), dc.fields(n, "int"))
        e.init_replicas(4, seed=SEED)
        e.set_temperatures(4.0)
        refused(sg, e, N.ERR_INVALID, "n_slices", 1, 3, 0.5)


def test_unsupported_problems(sg):
    from spin_glass_anneal_rl_amd import encoders as enc
    N = sg._native
    n = 24
    J, h = dc.couplings(n), dc.fields(n, "int")
    rng = np.random.RandomState(5)

    def ready(e):
        e.init_replicas(4, seed=SEED)
        e.set_temperatures(4.0)

    with sg.AnnealEngine(0) as e:  # CSR rows: the other call's
        e.set_csr(*dc.csr(n), h)
        ready(e)
        refused(sg, e, N.ERR_UNSUPPORTED, "sga_worldline_clusters serves", 1, 2, 0.5)
        e.worldline_clusters(1, 2, 0.5)
    dense_cases = {"integer valued": (J * np.float32(0.37), h), "zero diagonal": (J + np.eye(n, dtype=np.float32), h),
                   "symmetric": (np.triu(J) * 2 + np.tril(J), h), "2^24": (J * np.float32(1.0e6), h),
                   "multiples of 1/2": (J, h + np.float32(0.25))}
    for word, (Jx, hx) in dense_cases.items():
        with sg.AnnealEngine(0) as e:
            e.set_dense(np.ascontiguousarray(Jx, np.float32), hx.astype(np.float32))
            ready(e)
            refused(sg, e, N.ERR_UNSUPPORTED, word, 1, 2, 0.5)
    with sg.AnnealEngine(0) as e:  # stacked and shared batches
        e.set_dense_batch(np.stack([J, J]), np.stack([h, h]))
        ready(e)
        refused(sg, e, N.ERR_UNSUPPORTED, "batches", 1, 2, 0.5)
    with sg.AnnealEngine(0) as e:
        e.set_dense_shared(J, np.stack([h, h]))
        ready(e)
        refused(sg, e, N.ERR_UNSUPPORTED, "batches", 1, 2, 0.5)
    with sg.AnnealEngine(0) as e:  # ragged batch
        g = dc.csr(n)
        e.set_csr_batch([(g[0], g[1], g[2], h), (g[0], g[1], g[2], h)])
        ready(e)
        refused(sg, e, N.ERR_UNSUPPORTED, "ragged", 1, 2, 0.5)
    with sg.AnnealEngine(0) as e:  # implicit group couplings
        ng, mp, mem, c, hg = gc._assignment(6, 6)
        e.set_groups(ng, (mp, mem), c, hg)
        ready(e)
        refused(sg, e, N.ERR_UNSUPPORTED, "sga_set_groups", 1, 2, 0.5)
    with sg.AnnealEngine(0) as e:  # implicit TSP couplings
        xy = rng.rand(6, 2) * 100.0
        d32, A, B, ht, _ = enc.tsp_structure(np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1]), 200.0, 120.0,
                                             auto_scale=True)
        e.set_tsp(d32, A, B, ht)
        ready(e)
        refused(sg, e, N.ERR_UNSUPPORTED, "sga_set_tsp", 1, 2, 0.5)
    with engine(sg, n, "int", 4, 4.0) as e, engine(sg, n, "int", 4, 4.0) as twin:  # the rule is not looked at
        e.set_update_rule(N.RULE_GLAUBER)
        e.worldline_clusters_dense(1, 2, 0.5, round=0)
        twin.worldline_clusters_dense(1, 2, 0.5, round=0)
        assert_same_state(state(e), state(twin))


# ---- 9. the annealer ------------------------------------------------------------------------------------------------------------------------------
def test_simulated_quantum_annealing_run_with_dense_clusters(sg):
    n = 130
    rng = np.random.RandomState(130)
    J = np.triu(rng.randint(0, 2, (n, n)) * 2 - 1, 1).astype(np.float32)
    J = J + J.T
    model = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=False))
    model.set_couplings_from_matrix(torch.from_numpy(J))
    prob = oracle.Problem(J=J, h=np.zeros(n, np.float32))
    kw = dict(n_slices=8, n_instances=2, temperature=0.05, n_sweeps=60, seed=4242, measure_interval=10, dense_couplings=True,
              transverse_field=sg.TransverseField("linear_decrease", initial=3.0, final=0.05), cluster_interval=2)
    sqa = sg.SimulatedQuantumAnnealing(sg.SimulatedQuantumAnnealingConfig(dense_worldline_clusters=True, **kw))
    a = sqa.run(model)
    stats = sqa.cluster_statistics.copy()
    b = sqa.run(model)
    spins = a.best_configuration.numpy().astype(np.int8)
    assert set(np.unique(spins)) <= {-1, 1} and a.best_energy == oracle.energy(prob, spins)
    assert a.best_energy == b.best_energy and torch.equal(a.best_configuration, b.best_configuration)
    assert a.energy_history == b.energy_history and len(a.energy_history) == 6
    assert np.array_equal(stats, sqa.cluster_statistics)
    assert stats[0] >= 30 * n * 2 and stats[1] > 0 and stats[2] >= stats[1]  # 30 cluster sweeps of 2 instances
    # the flag off is the run as it was: a configuration that never mentions the flag, and run(dense_worldline_clusters=False)
    plain = sg.SimulatedQuantumAnnealing(sg.SimulatedQuantumAnnealingConfig(**kw))
    off = sg.SimulatedQuantumAnnealing(sg.SimulatedQuantumAnnealingConfig(dense_worldline_clusters=False, **kw))
    c, d, f = plain.run(model), off.run(model), sqa.run(model, dense_worldline_clusters=False)
    for r in (d, f):
        assert r.best_energy == c.best_energy and torch.equal(r.best_configuration, c.best_configuration)
        assert r.energy_history == c.energy_history and r.acceptance_rate_history == c.acceptance_rate_history
    assert plain.cluster_statistics is None and off.cluster_statistics is None and sqa.cluster_statistics is None
    assert a.energy_history != c.energy_history  # the cluster sweeps move the chain
    g = plain.run(model, dense_worldline_clusters=True)  # the keyword alone switches it on
    assert g.energy_history == a.energy_history and np.array_equal(plain.cluster_statistics, stats)
    # QuantumFluctuations passes the flag through
    base = sg.GPUAnnealer(sg.GPUAnnealerConfig(n_sweeps=30, final_temp=0.05, random_seed=7, record_interval=10))
    q = sg.QuantumFluctuations(base_annealer=base, transverse_field_schedule="linear_decrease", initial_field_strength=3.0,
                               dense_couplings=True, dense_worldline_clusters=True)
    r1 = q.simulated_quantum_anneal(model, n_trotter_slices=4, quantum_monte_carlo=True)
    assert r1.best_energy == oracle.energy(prob, r1.best_configuration.numpy().astype(np.int8))
    assert q.last.config.dense_worldline_clusters and q.last.cluster_statistics[0] >= 30 * n
