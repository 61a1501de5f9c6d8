"""Simulated quantum annealing on dense couplings on the device (sga_sweep_transverse_dense, csrc/sweep_transverse_clf.hip)
against the plain-Python specification of tests/transverse_reference.py over oracle.Problem(J=...): spins, energies,
bests and accept counters bit for bit (np.array_equal) on the shapes of tests/transverse_dense_cases.py -- n = 24 (less
than one window), 130 (just over one, padded rows), 300 (int32 fields), 1100 (several chunks and super-windows) -- with
h zero, integer and half-integer, int8 and fp32 rows, both arithmetics, 3 sweeps, at temperatures where 10 ... 40 % of the
proposals are accepted.  The reference runs are computed once per case and shared."""
import numpy as np
import pytest
import torch

import groups_cases as gc
import oracle
import transverse_dense_cases as dc
from test_cluster_moves_gpu import state

pytestmark = pytest.mark.gpu

NS, SEED = dc.NS, dc.SEED
STORAGES = ["i8", "f32"]
GRID = [(n, P, G) for n in dc.SMALL for P, G in dc.PG_SMALL] + [(n, P, G) for n in dc.LARGE for P, G in dc.PG_LARGE]
KEYS = ("S", "E", "acc", "be", "bs")


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def engine(sg, n, kind, R, T, storage="i8", cache="on", options=None, seed=SEED, s0=None, **replicas):
    e = sg.AnnealEngine(0)
    if options:
        e.set_options(options)
    e.set_field_cache(cache)
    e.set_dense(dc.couplings(n), dc.fields(n, kind), storage=storage)
    e.init_replicas(R, seed=seed, s0=s0, **replicas)
    e.set_temperatures(T)
    return e


def assert_matches(e, S, out):
    st = state(e)
    assert np.array_equal(st["S"], S)
    assert np.array_equal(st["E"], out["energy"])
    assert np.array_equal(st["acc"], out["n_accepted"])
    assert np.array_equal(st["be"], out["best_energy"])
    assert np.array_equal(st["bs"], out["best_spins"])


def assert_same_state(a, b, keys=KEYS):
    for key in keys:
        assert np.array_equal(a[key], b[key]), key


# ---- 1. against the reference, a different k per sweep and group ---------------------------------------------------------------
@pytest.mark.parametrize("arith", dc.ARITHS)
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("kind", dc.H_KINDS)
@pytest.mark.parametrize("n,P,G", GRID)
def test_against_the_reference(sg, n, P, G, kind, storage, arith):
    S, out = dc.reference(n, kind, P, G, arith)
    assert 0.10 <= dc.acceptance(n, out) <= 0.40  # every window holds accepts: it is evaluated again behind each
    with engine(sg, n, kind, P * G, dc.temps(n, P, G), storage) as e:
        e.sweep_transverse_dense(NS, P, dc.k_perp(G), arith=arith)
        lk = e.last_kernel()
        assert "sweep_transverse_clf_kernel" in lk and ("int8_t" if storage == "i8" else "float") in lk, lk
        assert ("int32_t" if n == 300 else "int16_t") in lk and ("f32 rule" if arith == oracle.ARITH_F32 else "f64 rule") in lk, lk
        assert_matches(e, S, out)
        assert e.counters() == (NS, 0) and np.array_equal(e.stats()[1], np.full(P * G, NS * n))
        # the tracked energies are the classical ones
        E = e.energies()
        e.recompute_energies()
        assert np.array_equal(e.energies(), E)
        assert np.array_equal(E, [oracle.energy(dc.problem(n, kind), r) for r in S])


# ---- 2. k = 0 is sga_sweep, bit for bit, whichever form the twin's sweep takes ---------------------------------------------------
@pytest.mark.parametrize("arith", dc.ARITHS)
@pytest.mark.parametrize("cache", ["on", "off"])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("n,P,G,kind", [(24, 6, 3, "half"), (130, 4, 3, "int"), (300, 4, 1, "half"), (1100, 2, 1, "zero")])
def test_k_zero_is_the_plain_sweep(sg, n, P, G, kind, storage, cache, arith):
    T = dc.temps(n, P, G)
    with engine(sg, n, kind, P * G, T, storage, cache) as e, engine(sg, n, kind, P * G, T, storage, cache) as twin:
        e.sweep_transverse_dense(NS, P, 0.0, arith=arith)
        twin.sweep(NS, arith=arith)
        assert ("sweep_clf" in twin.last_kernel()) == (cache == "on"), twin.last_kernel()
        assert_same_state(state(e), state(twin))
        assert state(e)["acc"].sum() > 0
        assert e.counters() == twin.counters()


# ---- 3. the same integer couplings held as CSR under sga_sweep_transverse ----------------------------------------------------------
@pytest.mark.parametrize("arith", dc.ARITHS)
@pytest.mark.parametrize("kind", ["int", "half"])
def test_csr_engine_walks_the_same_chain(sg, kind, arith):
    n, P, G = 130, 4, 3
    T, k = dc.temps(n, P, G), dc.k_perp(G)
    with engine(sg, n, kind, P * G, T, "f32") as e, sg.AnnealEngine(0) as c:
        c.set_csr(*dc.csr(n), dc.fields(n, kind))
        c.init_replicas(P * G, seed=SEED)
        c.set_temperatures(T)
        e.sweep_transverse_dense(NS, P, k, arith=arith)
        c.sweep_transverse(NS, P, k, arith=arith)
        assert "sweep_transverse_kernel" in c.last_kernel()
        assert_same_state(state(e), state(c))
        assert e.counters() == c.counters()


# ---- 4. the waves per slice do not show in the result --------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("waves", [1, 2, 8])
def test_waves_per_slice(sg, waves, storage):
    n, P, G, kind, arith = 1100, 4, 1, "half", oracle.ARITH_F64
    S, out = dc.reference(n, kind, P, G, arith)
    with engine(sg, n, kind, P * G, dc.temps(n, P, G), storage, options={"clf_waves": waves}) as e:
        e.sweep_transverse_dense(NS, P, dc.k_perp(G), arith=arith)
        assert "x %d wave(s)" % waves in e.last_kernel(), e.last_kernel()
        assert_matches(e, S, out)


def test_rows_streamed_past_the_first_batch(sg):
    """One wave over fp32 rows of six chunks: the sixth is streamed inside the field update (the TAIL build)."""
    n, P, G, kind, arith = 1400, 2, 1, "int", oracle.ARITH_F64
    S, out = dc.reference(n, kind, P, G, arith)
    assert 0.10 <= dc.acceptance(n, out) <= 0.40
    with engine(sg, n, kind, P * G, dc.temps(n, P, G), "f32", options={"clf_waves": 1}) as e:
        e.sweep_transverse_dense(NS, P, dc.k_perp(G), arith=arith)
        assert "TAIL=1" in e.last_kernel() and "x 1 wave(s)" in e.last_kernel(), e.last_kernel()
        assert_matches(e, S, out)


# ---- 5. one call of 2 sweeps equals two calls of 1 sweep ------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", dc.ARITHS)
@pytest.mark.parametrize("n,P,G,storage", [(24, 2, 3, "i8"), (130, 6, 3, "f32"), (300, 4, 1, "i8"), (1100, 2, 1, "f32")])
def test_two_sweeps_are_two_calls(sg, n, P, G, storage, arith):
    k, T = dc.k_perp(G)[:2], dc.temps(n, P, G)
    with engine(sg, n, "half", P * G, T, storage) as e, engine(sg, n, "half", P * G, T, storage) as twin:
        e.sweep_transverse_dense(2, P, k, arith=arith)
        twin.sweep_transverse_dense(1, P, k[:1], arith=arith)
        twin.sweep_transverse_dense(1, P, k[1:], arith=arith)
        assert_same_state(state(e), state(twin))
        assert e.counters() == twin.counters() == (2, 0)


# ---- 6. a rank that holds whole groups ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,P,storage", [(24, 2, "f32"), (130, 6, "i8"), (130, 4, "f32")])
def test_sharded_groups(sg, n, P, storage):
    G, k = 3, dc.k_perp(3)
    T = dc.temps(n, P, G)
    S, out = dc.reference(n, "int", P, G, oracle.ARITH_F64)
    with engine(sg, n, "int", P * G, T, storage) as full:
        full.sweep_transverse_dense(NS, P, k)
        want = state(full)
        assert np.array_equal(want["S"], S)
    for g0, gn in ((1, 2), (2, 1)):  # the last two groups, the last one
        lo, R = g0 * P, gn * P
        with engine(sg, n, "int", R, T[lo:], storage, R_global=P * G, replica0=lo) as part:
            part.sweep_transverse_dense(NS, P, k[:, g0:])
            got = state(part)
            for key in KEYS:
                assert np.array_equal(got[key], want[key][lo:lo + R]), key


# ---- 7. T = 0 and T = inf -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", dc.ARITHS)
@pytest.mark.parametrize("n,P,storage", [(130, 4, "i8"), (24, 2, "f32")])
def test_temperature_limits(sg, n, P, storage, arith):
    import transverse_reference as tr
    G, kind = 3, "half"
    T = np.repeat([0.0, np.inf, dc.SHAPE[n]["T0"]], P)
    k = dc.k_perp(G)
    S = oracle.init_spins(n, P * G, SEED)
    out = tr.sweeps(dc.problem(n, kind), S, T, NS, P, k, arith=arith, seed=SEED)
    with engine(sg, n, kind, P * G, T, storage) as e:
        e.sweep_transverse_dense(NS, P, k, arith=arith)
        assert_matches(e, S, out)
    assert np.all(out["n_accepted"][P:2 * P] == NS * n)  # T = inf accepts everything
    assert np.all(out["n_accepted"][:P] < NS * n)


# ---- 8. identical slices under a large coupling are frozen ---------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", dc.ARITHS)
@pytest.mark.parametrize("n,P,G,storage", [(24, 2, 1, "i8"), (130, 6, 3, "f32"), (300, 4, 1, "i8")])
def test_frozen_slices(sg, n, P, G, storage, arith):
    s0 = np.repeat(oracle.init_spins(n, 1, SEED), P * G, axis=0)
    with engine(sg, n, "int", P * G, 1.0, storage, s0=s0) as e:
        before = state(e)
        e.sweep_transverse_dense(NS, P, 1.0e4, arith=arith)
        after = state(e)
        assert np.array_equal(after["S"], s0) and not after["acc"].any()
        assert_same_state(before, after)


# ---- 9. what moves and what does not ---------------------------------------------------------------------------------------------------------
def test_counters_ladder_and_exchange_statistics(sg):
    n, P, G = 130, 4, 3
    with engine(sg, n, "int", P * G, 1.0) as e:
        e.set_ladder(np.tile(np.asarray([0.5, 1.0, 2.0, 4.0]) * dc.SHAPE[n]["T0"], G), n_ladders=G)
        e.sweep(2)
        e.exchange()
        e.exchange()
        slot, stats, T = e.slot_map(), e.exchange_stats(), e.temperatures()
        assert stats[0].sum() > 0 and e.counters() == (2, 2)
        e.sweep_transverse_dense(NS, P, 0.25)
        assert e.counters() == (2 + NS, 2)
        assert np.array_equal(e.slot_map(), slot) and np.array_equal(e.temperatures(), T)
        assert all(np.array_equal(a, b) for a, b in zip(e.exchange_stats(), stats))
        assert np.array_equal(e.stats()[1], np.full(P * G, (2 + NS) * n))
        assert "sweep_transverse_clf_kernel" in e.last_kernel()
        e.sweep_transverse_dense(0, P, 0.25)  # a no-op
        assert e.counters() == (2 + NS, 2)


# ---- 10. the cached fields stay valid ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("n,kind", [(130, "half"), (300, "int")])
def test_fields_stay_valid(sg, n, kind, storage):
    """A cached sweep(2) after the call goes on from the fields the call wrote back: against a twin that is given the
    spins by set_spins and seeds its fields from them."""
    P, G = 4, 3 if n == 130 else 1
    T = dc.temps(n, P, G)
    with engine(sg, n, kind, P * G, T, storage) as e, engine(sg, n, kind, P * G, T, storage) as twin:
        e.sweep(1)
        assert "sweep_clf" in e.last_kernel()  # the fields are resident and valid now
        e.sweep_transverse_dense(2, P, dc.k_perp(G)[:2])
        mid = state(e)
        assert mid["acc"].sum() > 0
        for r in range(P * G):
            twin.set_spins(r, mid["S"][r])
        twin.set_counters(*e.counters())
        assert np.array_equal(twin.energies(), mid["E"])
        e.sweep(2)
        twin.sweep(2)
        assert "sweep_clf" in e.last_kernel()
        a, b = state(e), state(twin)
        assert np.array_equal(a["S"], b["S"]) and np.array_equal(a["E"], b["E"])
        e.recompute_energies()
        assert np.array_equal(e.energies(), a["E"])


@pytest.mark.parametrize("cache", ["off", "auto"])
@pytest.mark.parametrize("storage", STORAGES)
def test_the_call_seeds_the_fields_after_an_uncached_sweep(sg, storage, cache):
    """Cache off: the row kernels move the spins only.  Cache auto: replicas are routed one by one, so the call seeds the
    fields itself whatever the flag says."""
    n, kind, P, G = 130, "half", 4, 3
    T, k = dc.temps(n, P, G), dc.k_perp(G)
    with engine(sg, n, kind, P * G, T, storage, cache=cache) as e, engine(sg, n, kind, P * G, T, storage, cache="on") as twin:
        e.sweep(1)
        twin.sweep(1)
        assert ("sweep_clf" not in e.last_kernel() or cache == "auto") and "sweep_clf" in twin.last_kernel()
        e.sweep_transverse_dense(NS, P, k)
        twin.sweep_transverse_dense(NS, P, k)
        assert_same_state(state(e), state(twin))
        e.sweep(1)  # (the row kernels again: they move the spins only)
        twin.sweep(1)
        e.sweep_transverse_dense(1, P, k[:1])
        twin.sweep_transverse_dense(1, P, k[:1])
        assert_same_state(state(e), state(twin))


# ---- 11. refusals leave the engine as it was ---------------------------------------------------------------------------------------------------------
def refused(sg, e, code, word, *args, **kw):
    ragged = getattr(e, "_sizes", None) is not None  # (best(r) of a ragged batch has the model's own length)
    before = dict(S=e.spins(), E=e.energies(), acc=e.stats()[0]) if ragged else state(e)
    counters = e.counters()
    with pytest.raises(sg.AnnealingError) as err:
        e.sweep_transverse_dense(*args, **kw)
    assert err.value.details["code"] == code and word in str(err.value), str(err.value)
    now = dict(S=e.spins(), E=e.energies(), acc=e.stats()[0]) if ragged else state(e)
    assert all(np.array_equal(now[key], before[key]) for key in before)
    assert e.counters() == counters


def test_invalid_calls(sg):
    N = sg._native
    n = 24
    with engine(sg, n, "int", 12, 4.0) as e:
        e.sweep(1)
        for P in (1, 0, -2, 3, 5, 8, 24):
            refused(sg, e, N.ERR_INVALID, "n_slices", 1, P, 0.25)
        refused(sg, e, N.ERR_INVALID, "n_sweeps", -1, 4, 0.25)
        refused(sg, e, N.ERR_INVALID, "arith", 1, 4, 0.25, arith=7)
        for bad in (np.nan, np.inf, -np.inf, [[0.25, 0.25, np.nan]]):
            refused(sg, e, N.ERR_INVALID, "k_perp", 1, 4, bad)
        assert N.lib().sga_sweep_transverse_dense(e._h, 1, 4, N.ARITH_F64, None) == N.ERR_INVALID
        k = np.zeros(3, np.float32)
        assert N.lib().sga_sweep_transverse_dense(None, 1, 4, N.ARITH_F64, k.ctypes.data) == N.ERR_INVALID
        dev = torch.zeros(3, dtype=torch.float32, device="cuda")
        assert N.lib().sga_sweep_transverse_dense(e._h, 1, 4, N.ARITH_F64, dev.data_ptr()) == N.ERR_INVALID
        assert e.counters() == (1, 0)
    with engine(sg, n, "int", 8, 4.0, R_global=16, replica0=6) as e:  # replica0 % 4 != 0
        refused(sg, e, N.ERR_INVALID, "replica0", 1, 4, 0.25)
        e.sweep_transverse_dense(1, 2, 0.25)  # 6 % 2 == 0
    with sg.AnnealEngine(0) as e:
        with pytest.raises(sg.AnnealingError, match="no couplings"):
            e.sweep_transverse_dense(1, 2, 0.25)
        e.set_dense(dc.couplings(n), dc.fields(n, "int"))
        with pytest.raises(sg.AnnealingError, match="no replicas"):
            e.sweep_transverse_dense(1, 2, 0.25)
    with sg.AnnealEngine(0) as e:  # an argument error comes before the problem's kind
        e.set_csr(*dc.csr(n), dc.fields(n, "int"))
        e.init_replicas(4, seed=SEED)
        e.set_temperatures(4.0)
        refused(sg, e, N.ERR_INVALID, "n_slices", 1, 3, 0.25)


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
        refused(sg, e, N.ERR_UNSUPPORTED, "sga_sweep_transverse serves", 1, 2, 0.25)
        e.sweep_transverse(1, 2, 0.25)
    with sg.AnnealEngine(0) as e:  # a sparse matrix that sga_set_dense kept as CSR
        A = np.zeros((256, 256), np.float32)
        for i in range(256):
            A[i, (i + 1) % 256] = A[(i + 1) % 256, i] = 1.0
        e.set_field_cache("off")
        e.set_dense(A, np.zeros(256, np.float32))
        ready(e)
        if e.route_query().kind == N.ROUTE_CSR:
            refused(sg, e, N.ERR_UNSUPPORTED, "sga_sweep_transverse serves", 1, 2, 0.25)
        else:
            e.sweep_transverse_dense(1, 2, 0.25)
    dense_cases = {"integer valued": (J * np.float32(0.37), h), "zero diagonal": (J + np.eye(n, dtype=np.float32), h),
                   "symmetric": (np.triu(J) * 2 + np.tril(J), h), "2^24": (J * np.float32(1.0e6), h),
                   "multiples of 1/2": (J, h + np.float32(0.25))}
    for word, (Jx, hx) in dense_cases.items():
        with sg.AnnealEngine(0) as e:
            e.set_dense(np.ascontiguousarray(Jx, np.float32), hx.astype(np.float32))
            ready(e)
            refused(sg, e, N.ERR_UNSUPPORTED, word, 1, 2, 0.25)
    with sg.AnnealEngine(0) as e:  # stacked and shared batches
        e.set_dense_batch(np.stack([J, J]), np.stack([h, h]))
        ready(e)
        refused(sg, e, N.ERR_UNSUPPORTED, "batches", 1, 2, 0.25)
    with sg.AnnealEngine(0) as e:
        e.set_dense_shared(J, np.stack([h, h]))
        ready(e)
        refused(sg, e, N.ERR_UNSUPPORTED, "batches", 1, 2, 0.25)
    with sg.AnnealEngine(0) as e:  # ragged batch
        g = dc.csr(n)
        e.set_csr_batch([(g[0], g[1], g[2], h), (g[0], g[1], g[2], h)])
        ready(e)
        refused(sg, e, N.ERR_UNSUPPORTED, "ragged", 1, 2, 0.25)
    with sg.AnnealEngine(0) as e:  # implicit group couplings
        ng, mp, mem, c, hg = gc._assignment(6, 6)
        e.set_groups(ng, (mp, mem), c, hg)
        ready(e)
        refused(sg, e, N.ERR_UNSUPPORTED, "sga_set_groups", 1, 2, 0.25)
    with sg.AnnealEngine(0) as e:  # implicit TSP couplings
        xy = rng.rand(6, 2) * 100.0
        d32, A, B, ht, _ = enc.tsp_structure(np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1]), 200.0, 120.0,
                                             auto_scale=True)
        e.set_tsp(d32, A, B, ht)
        ready(e)
        refused(sg, e, N.ERR_UNSUPPORTED, "sga_set_tsp", 1, 2, 0.25)
    with engine(sg, n, "int", 4, 4.0) as e:  # another rule
        e.set_update_rule(N.RULE_GLAUBER)
        refused(sg, e, N.ERR_UNSUPPORTED, "Metropolis", 1, 2, 0.25)
        e.set_update_rule(N.RULE_METROPOLIS)
        e.sweep_transverse_dense(1, 2, 0.25)


# ---- 12. the annealer ---------------------------------------------------------------------------------------------------------------------------------
def test_simulated_quantum_annealing_run_on_a_dense_model(sg):
    n = 64
    rng = np.random.RandomState(64)
    J = np.triu(rng.randint(0, 2, (n, n)) * 2 - 1, 1).astype(np.float32)
    J = J + J.T
    model = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=False))
    model.set_couplings_from_matrix(torch.from_numpy(J))
    prob = oracle.Problem(J=J, h=np.zeros(n, np.float32))
    cfg = sg.SimulatedQuantumAnnealingConfig(n_slices=8, n_instances=2, temperature=0.05, n_sweeps=60,
                                             transverse_field=sg.TransverseField("linear_decrease", initial=3.0, final=0.05),
                                             seed=4242, measure_interval=10, dense_couplings=True)
    sqa = sg.SimulatedQuantumAnnealing(cfg)
    a = sqa.run(model, measure_overlaps=True)
    b = sg.SimulatedQuantumAnnealing(cfg).run(model)
    spins = a.best_configuration.numpy().astype(np.int8)
    assert set(np.unique(spins)) <= {-1, 1} and a.best_energy == oracle.energy(prob, spins)
    assert a.best_energy == b.best_energy and torch.equal(a.best_configuration, b.best_configuration)
    assert a.energy_history == b.energy_history and len(a.energy_history) == 6
    assert a.best_energy <= min(a.energy_history)
    assert a.algorithm == "simulated_quantum_annealing" and a.n_sweeps == 60
    assert sqa.final_energies.shape == (2, 8) and sqa.slice_overlaps.shape == (16, 16)
    assert np.all(np.diag(sqa.slice_overlaps) == n)
    assert max(a.acceptance_rate_history) > 0.0
    # the same model without the flag is still refused with the engine's reason: no classical fallback
    plain = sg.SimulatedQuantumAnnealingConfig(n_slices=8, n_instances=2, temperature=0.05, n_sweeps=60, seed=4242)
    with pytest.raises(sg.AnnealingError, match="dense"):
        sg.SimulatedQuantumAnnealing(plain).run(model)
    # world-line clusters are not served on dense rows
    with pytest.raises(sg.AnnealingError, match="world-line clusters are not served on dense couplings"):
        sqa.run(model, worldline_clusters=True)
    # the upstream README's two calls
    base = sg.GPUAnnealer(sg.GPUAnnealerConfig(n_sweeps=30, final_temp=0.05, random_seed=7, record_interval=10))
    q = sg.QuantumFluctuations(base_annealer=base, transverse_field_schedule="linear_decrease", initial_field_strength=3.0,
                               dense_couplings=True)
    r1 = q.simulated_quantum_anneal(model, n_trotter_slices=4, quantum_monte_carlo=True)
    r2 = q.path_integral_mc(model, imaginary_time_slices=6, quantum_temperature=0.1)
    for r in (r1, r2):
        assert r.best_energy == oracle.energy(prob, r.best_configuration.numpy().astype(np.int8))
    q0 = sg.QuantumFluctuations(base_annealer=base, transverse_field_schedule="linear_decrease", initial_field_strength=3.0)
    with pytest.raises(sg.AnnealingError, match="dense"):
        q0.simulated_quantum_anneal(model, n_trotter_slices=4)
