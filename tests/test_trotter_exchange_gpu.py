"""Time links and the exchange between Trotter groups along the transverse field on the device (sga_get_time_links,
sga_exchange_transverse, csrc/trotter_exchange.hip) against the plain-Python specification of
tests/trotter_exchange_reference.py: counts, spins, energies, bests, flags bit for bit (np.array_equal).

Counts: n = 5 (one lane), 24, 130, 1100 (two site chunks) and 1025 -- one site beyond the 1024 sites of one workgroup of the
count kernel as built (TIME_LINKS_CHUNK_SITES, 64 lanes x 16 bytes) --, P in {2, 3, 4, 64}, G in {1, 3}, on rings after two
sweeps, on the CSR shapes of tests/test_transverse_gpu.py and the dense cases of tests/transverse_dense_cases.py after two
transverse sweeps, and on made states.  The exchange: the cases of tests/trotter_exchange_cases.py, whose coverage (a
swap at prob < 1, a refusal) is asserted on the reference here.  test_composition_* are the ones that a right decision
with a wrong swap of the field rows cannot pass."""
import numpy as np
import pytest
import torch

import oracle
import test_transverse_gpu as tg
import transverse_dense_cases as dc
import transverse_reference as tr
import trotter_exchange_cases as xc
import trotter_exchange_reference as xr
import worldline_reference as wr
from test_cluster_moves_gpu import csr_from_edges, state
from test_transverse_dense_gpu import engine as dense_engine

pytestmark = pytest.mark.gpu

SEED = xc.SEED
CHUNK = 1024  # TIME_LINKS_CHUNK_SITES of csrc/sga_quantum.h
KEYS = ("S", "E", "acc", "be", "bs")


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def ring_engine(sg, n, R, s0=None, seed=SEED):
    rng = np.random.RandomState(n)
    graph = csr_from_edges(n, [(i, (i + 1) % n, float(rng.randint(0, 2) * 2 - 1)) for i in range(n)])
    e = sg.AnnealEngine(0)
    e.set_csr(*graph, np.zeros(n, np.float32))
    e.init_replicas(R, seed=seed, s0=s0)
    e.set_temperatures(2.0)
    return e


def assert_counts(e, P):
    """time_links onto the host and into a device tensor, against the count of e.spins()."""
    want = xr.time_links(e.spins(), P)
    got = e.time_links(P)
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)
    assert "time_links_kernel" in e.last_kernel() and "%d slices" % P in e.last_kernel()
    out = torch.full((len(want),), -7, dtype=torch.int64, device="cuda")
    assert e.time_links(P, out=out) is out
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    return want


def assert_applied(e, want):
    st = state(e)
    assert np.array_equal(st["S"], want["spins"])
    assert np.array_equal(st["E"], want["energy"])
    assert np.array_equal(st["be"], want["best_energy"])
    assert np.array_equal(st["bs"], want["best_spins"])


# ---- 1. the counts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 24, 130, 1100, CHUNK + 1])
def test_counts_on_rings(sg, n):
    seen = set()
    for P in (2, 3, 4, 64):
        for G in (1, 3):
            with ring_engine(sg, n, P * G) as e:
                if P % 2 == 0:
                    e.sweep_transverse(2, P, 0.5)
                else:
                    e.sweep(2)
                B = assert_counts(e, P)
                assert np.all(B % 2 == 0) and np.all(B >= 0) and np.all(B <= n * P)  # (n = 5, P = 2: 0 does occur)
                seen.update(B.tolist())
                assert e.counters() == (2, 0)
    assert len(seen) > 4


@pytest.mark.parametrize("name", ["lattice3", "lattice6", "random300"])
@pytest.mark.parametrize("P,G", [(2, 3), (4, 1), (64, 1)])
def test_counts_after_transverse_sweeps_csr(sg, name, P, G):
    with tg.engine(sg, name, P * G, tg.temps(P, G)) as e:
        e.sweep_transverse(2, P, tg.couplings(G)[:2])
        before = state(e)
        assert_counts(e, P)
        after = state(e)
        assert all(np.array_equal(before[key], after[key]) for key in KEYS)  # read only


@pytest.mark.parametrize("storage", ["i8", "f32"])
@pytest.mark.parametrize("n,P,G", [(24, 2, 3), (130, 4, 3), (1100, 4, 1)])
def test_counts_after_transverse_sweeps_dense(sg, n, P, G, storage):
    with dense_engine(sg, n, "half", P * G, dc.temps(n, P, G), storage) as e:
        e.sweep_transverse_dense(2, P, dc.k_perp(G)[:2])
        assert_counts(e, P)
        e.sweep_transverse_dense(1, P, dc.k_perp(G)[2:])  # the fields are still the sweep's: the chain of three sweeps
        S, out = dc.reference(n, "half", P, G, oracle.ARITH_F64)
        assert np.array_equal(e.spins(), S) and np.array_equal(e.energies(), out["energy"])


@pytest.mark.parametrize("n", [5, 130, CHUNK + 1])
def test_counts_of_made_states(sg, n):
    s = oracle.init_spins(n, 1, SEED)[0]
    for P in (2, 3, 4, 64):
        same = np.repeat(s[None, :], P, axis=0)
        one = same.copy()
        one[P - 1, n - 1] *= -1  # the last site: the last lane that holds one
        states = [(same, 0), (one, 2)]
        if P % 2 == 0:
            states.append((np.stack([s if p % 2 == 0 else -s for p in range(P)]), n * P))
        s0 = np.concatenate([x for x, _ in states]).astype(np.int8)
        with ring_engine(sg, n, len(s0), s0=s0) as e:
            assert np.array_equal(assert_counts(e, P), [b for _, b in states])
    differ = np.stack([s, s]).astype(np.int8)
    differ[1, 0] *= -1
    with ring_engine(sg, n, 2, s0=differ) as e:  # P = 2 with one differing site: both links of the ring
        assert np.array_equal(assert_counts(e, 2), [2])


# ---- 2. the exchange against the reference -------------------------------------------------------------------------------------------
def test_the_cases_cover_a_swap_below_one_and_a_refusal():
    partial, refused, sure = xc.coverage()
    assert partial >= 1 and refused >= 1 and sure >= 1, (partial, refused, sure)
    assert (partial, refused, sure) == (1, 3, 8)
    probs = [d["prob"] for G in xc.GROUPS for lad in xc.LADDERS for par in xc.PARITIES for d in xc.after(G, lad, par)["decisions"]]
    assert any(0.0 < p < 1.0 for p in probs)


@pytest.mark.parametrize("parity", xc.PARITIES)
@pytest.mark.parametrize("ladder", xc.LADDERS)
@pytest.mark.parametrize("G", xc.GROUPS)
def test_exchange_against_the_reference(sg, G, ladder, parity):
    P = xc.P
    S, out = xc.before(G, ladder)
    want = xc.after(G, ladder, parity)
    k = xc.k_ladder(G)
    with tg.engine(sg, xc.NAME, P * G, xc.temps(G, ladder), seed=SEED) as e:
        e.sweep_transverse(xc.NS, P, np.repeat(k[None, :], xc.NS, axis=0))
        tg.assert_matches(e, S, out)
        acc, att, T, counters = e.stats()[0], e.stats()[1], e.temperatures(), e.counters()
        accepted, links = e.exchange_transverse(P, k, parity=parity, round=xc.ROUND)
        assert "trotter_exchange_kernel" in e.last_kernel() and "%d slices" % P in e.last_kernel()
        assert accepted.dtype == np.int32 and np.array_equal(accepted, want["accepted"])
        assert links.dtype == np.int64 and np.array_equal(links, want["links"])
        assert_applied(e, want)
        # what does not move
        assert np.array_equal(e.stats()[0], acc) and np.array_equal(e.stats()[1], att)
        assert np.array_equal(e.temperatures(), T) and e.counters() == counters
        E = e.energies()
        e.recompute_energies()
        assert np.array_equal(e.energies(), E)


def test_round_and_parity_defaults(sg):
    """round None is counters()[0], parity None is round & 1."""
    P, G, ladder = xc.P, 4, "k"
    k = xc.k_ladder(G)
    with tg.engine(sg, xc.NAME, P * G, xc.temps(G, ladder), seed=SEED) as e, tg.engine(sg, xc.NAME, P * G, xc.temps(G, ladder), seed=SEED) as twin:
        for x in (e, twin):
            x.sweep_transverse(3, P, 1.0)
        a = e.exchange_transverse(P, k)
        b = twin.exchange_transverse(P, k, parity=1, round=3)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0][0] == 0 and a[0][3] == 0
        assert all(np.array_equal(u, v) for u, v in zip(state(e).values(), state(twin).values()))
        c = e.exchange_transverse(P, 1.0, round=6)  # a scalar k, parity 0: x = 0 for every pair
        assert np.array_equal(c[0], [1, 1, 1, 1])


# ---- 3. limits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("G", [1, 2, 3, 4])
def test_equal_k_and_T_swaps_every_pair(sg, G, parity):
    P = 4
    with tg.engine(sg, "lattice6", P * G, 2.0, seed=SEED) as e:
        e.sweep_transverse(1, P, 0.5)
        st = state(e)
        want = xr.apply(st["S"], st["E"], st["be"], st["bs"], np.full(P * G, 2.0), np.full(G, 0.5, np.float32), P, parity, SEED, 3)
        assert all(d["swap"] and d["x"] == 0.0 for d in want["decisions"])
        accepted, links = e.exchange_transverse(P, 0.5, parity=parity, round=3)
        assert np.array_equal(accepted, want["accepted"]) and accepted.sum() == 2 * len(xr.pairs(G, parity))
        assert np.array_equal(links, want["links"])
        assert_applied(e, want)


@pytest.mark.parametrize("bad", [0.0, np.inf])
def test_unusable_temperature_leaves_its_pairs_alone(sg, bad):
    P, G = 2, 4
    T = np.repeat([2.0, bad, 2.0, 2.0], P)
    with tg.engine(sg, "lattice3", P * G, T, seed=SEED) as e:
        st = state(e)
        want = xr.apply(st["S"], st["E"], st["be"], st["bs"], T, np.full(G, 0.5, np.float32), P, 0, SEED, 0)
        accepted, _ = e.exchange_transverse(P, 0.5, parity=0, round=0)
        assert np.array_equal(accepted, [0, 0, 1, 1]) and np.array_equal(accepted, want["accepted"])
        assert_applied(e, want)
        accepted, _ = e.exchange_transverse(P, 0.5, parity=1, round=0)  # the pair (1, 2): group 1 is the unusable one
        assert not accepted.any()
        assert_applied(e, want)


# ---- 4. composition: the fields travel with the spins ----------------------------------------------------------------------------------------
def compose(prob, cprob, S, T, P, G, kseq, pb):
    """sweeps(2), exchange, sweeps(2), clusters(1), exchange on the references; returns the state and the two rounds."""
    out = tr.sweeps(prob, S, T, 2, P, kseq[:2], seed=SEED)
    x1 = xr.apply(S, out["energy"], out["best_energy"], out["best_spins"], T, kseq[1], P, 0, SEED, 1)
    S[:] = x1["spins"]
    out = tr.sweeps(prob, S, T, 2, P, kseq[2:4], seed=SEED, sweep0=2, energy=x1["energy"], best_energy=x1["best_energy"],
                    best_spins=x1["best_spins"])
    cl = wr.sweeps(cprob, S, T, 1, P, pb, seed=SEED, round=3, energy=out["energy"], best_energy=out["best_energy"],
                   best_spins=out["best_spins"])
    x2 = xr.apply(S, cl["energy"], cl["best_energy"], cl["best_spins"], T, kseq[3], P, 1, SEED, 3)
    S[:] = x2["spins"]
    return x1, x2


def run_composition(e, P, kseq, pb, dense):
    sweep = e.sweep_transverse_dense if dense else e.sweep_transverse
    move = e.worldline_clusters_dense if dense else e.worldline_clusters
    sweep(2, P, kseq[:2])
    a1, _ = e.exchange_transverse(P, kseq[1], parity=0, round=1)
    sweep(2, P, kseq[2:4])
    move(1, P, pb, round=3)
    a2, _ = e.exchange_transverse(P, kseq[3], parity=1, round=3)
    return a1, a2


def composition_inputs(G):
    kseq = np.repeat((1.0 + 0.02 * np.arange(G)).astype(np.float32)[None, :], 4, axis=0)
    return kseq, np.full((1, G), 0.6)


@pytest.mark.parametrize("storage", ["i8", "f32"])
def test_composition_on_dense_rows(sg, storage):
    n, kind, P, G = 130, "half", 4, 3
    T = np.full(P * G, dc.SHAPE[n]["T0"])
    kseq, pb = composition_inputs(G)
    S = oracle.init_spins(n, P * G, SEED)
    x1, x2 = compose(dc.problem(n, kind), dc.problem(n, kind, as_csr=True), S, T, P, G, kseq, pb)
    assert x1["accepted"].any() and x2["accepted"].any()  # rows do trade places, in both rounds
    with dense_engine(sg, n, kind, P * G, T, storage, seed=SEED) as e:
        a1, a2 = run_composition(e, P, kseq, pb, dense=True)
        assert np.array_equal(a1, x1["accepted"]) and np.array_equal(a2, x2["accepted"])
        assert "fields traded" in e.last_kernel()
        assert_applied(e, x2)
        e.sweep(1)  # cached: it goes on from the fields as they were traded
        assert "sweep_clf" in e.last_kernel()
        ref = oracle.sweeps(dc.problem(n, kind), S, T, 1, seed=SEED, sweep0=4, energy=x2["energy"], best_energy=x2["best_energy"])
        assert np.array_equal(e.spins(), S) and np.array_equal(e.energies(), ref["energy"])
        assert np.array_equal(state(e)["be"], ref["best_energy"])
        E = e.energies()
        e.recompute_energies()
        assert np.array_equal(e.energies(), E)


def test_composition_on_csr_rows(sg):
    name, P, G = "lattice6", 4, 3
    g, h = tg.shape(name)
    prob = oracle.Problem(csr=g, h=h)
    T = np.full(P * G, 1.5)
    kseq, pb = composition_inputs(G)
    S = oracle.init_spins(prob.n, P * G, SEED)
    x1, x2 = compose(prob, prob, S, T, P, G, kseq, pb)
    assert x1["accepted"].any() and x2["accepted"].any()
    with tg.engine(sg, name, P * G, T, cache="on", seed=SEED) as e:
        a1, a2 = run_composition(e, P, kseq, pb, dense=False)
        assert np.array_equal(a1, x1["accepted"]) and np.array_equal(a2, x2["accepted"])
        assert_applied(e, x2)
        e.sweep(1)
        ref = oracle.sweeps(prob, S, T, 1, seed=SEED, sweep0=4, energy=x2["energy"], best_energy=x2["best_energy"])
        assert np.array_equal(e.spins(), S) and np.array_equal(e.energies(), ref["energy"])


def test_csr_fields_travel_when_they_are_valid(sg):
    """A cached CSR sweep leaves valid fields; exchange; a cached sweep goes on from them -- against a twin that is given
    the spins by set_spins and seeds its fields from them."""
    name, P, G = "lattice6", 4, 2
    with tg.engine(sg, name, P * G, 2.0, cache="on", seed=SEED) as e, tg.engine(sg, name, P * G, 2.0, cache="on", seed=SEED) as twin:
        e.sweep(2)
        assert "sweep_clf_csr_kernel" in e.last_kernel()
        accepted, _ = e.exchange_transverse(P, 0.5, parity=0, round=2)
        assert np.array_equal(accepted, [1, 1]) and "fields traded" in e.last_kernel()
        mid = state(e)
        for r in range(P * G):
            twin.set_spins(r, mid["S"][r])
        twin.set_counters(*e.counters())
        assert np.array_equal(twin.energies(), mid["E"])
        e.sweep(2)
        twin.sweep(2)
        a, b = state(e), state(twin)
        assert np.array_equal(a["S"], b["S"]) and np.array_equal(a["E"], b["E"])


# ---- 5. what does not move; refusals ----------------------------------------------------------------------------------------------------------
def test_ladder_statistics_and_counters_do_not_move(sg):
    name, P, G = "lattice6", 4, 3
    with tg.engine(sg, name, P * G, 1.0, seed=SEED) as e:
        e.set_ladder(np.tile([0.5, 1.0, 2.0, 4.0], G), n_ladders=G)
        e.sweep(2)
        e.exchange()
        slot, stats, T, counters, acc = e.slot_map(), e.exchange_stats(), e.temperatures(), e.counters(), e.stats()
        B = e.time_links(P)
        accepted, links = e.exchange_transverse(P, [0.5, 0.5, 0.5], parity=0, round=9)
        assert np.array_equal(links, B)
        assert np.array_equal(e.slot_map(), slot) and np.array_equal(e.temperatures(), T) and e.counters() == counters
        assert all(np.array_equal(a, b) for a, b in zip(e.exchange_stats(), stats))
        assert all(np.array_equal(a, b) for a, b in zip(e.stats(), acc))


def test_refusals_leave_everything_as_it_was(sg):
    N = sg._native
    P, G = 4, 3
    with tg.engine(sg, "lattice6", P * G, 2.0, seed=SEED) as e:
        e.sweep_transverse(1, P, 0.5)
        before, counters = state(e), e.counters()
        calls = [(lambda: e.exchange_transverse(P, 0.5, parity=2, round=0), N.ERR_INVALID, "parity must be 0 or 1"),
                 (lambda: e.exchange_transverse(P, np.nan, parity=0, round=0), N.ERR_INVALID, "NaN"),
                 (lambda: e.exchange_transverse(5, 0.5, parity=0, round=0), N.ERR_INVALID, "n_slices must divide"),
                 (lambda: e.time_links(5), N.ERR_INVALID, "n_slices must divide"),
                 (lambda: e.time_links(1), N.ERR_INVALID, "at least 2")]
        for call, code, word in calls:
            with pytest.raises(sg.AnnealingError) as err:
                call()
            assert err.value.details["code"] == code and word in str(err.value), str(err.value)
            now = state(e)
            assert all(np.array_equal(now[key], before[key]) for key in KEYS) and e.counters() == counters
        with pytest.raises(sg.AnnealingError, match="scalar or"):
            e.exchange_transverse(P, [0.5, 0.5], parity=0, round=0)
        with pytest.raises(sg.AnnealingError, match="int64 CUDA tensor"):
            e.time_links(P, out=torch.zeros(G, dtype=torch.int32, device="cuda"))
    with tg.engine(sg, "lattice6", P, 2.0, seed=SEED, R_global=P * G, replica0=P) as part:  # a shard: the counts are served
        assert part.time_links(P).shape == (1,)
        with pytest.raises(sg.AnnealingError, match="R_local == R_global") as err:
            part.exchange_transverse(P, 0.5, parity=0, round=0)
        assert err.value.details["code"] == N.ERR_INVALID
    g, h = tg.shape("lattice6")  # a batch is not served
    with sg.AnnealEngine(0) as e:
        e.set_csr_shared(*g, np.stack([h, -h]))
        e.init_replicas(8, seed=1)
        e.set_temperatures(1.0)
        for call, what in ((lambda: e.time_links(2), "time links"), (lambda: e.exchange_transverse(2, 0.5, parity=0, round=0), "transverse-field exchanges")):
            with pytest.raises(sg.AnnealingError, match=what + " are not implemented for many-model batches") as err:
                call()
            assert err.value.details["code"] == N.ERR_UNSUPPORTED


# ---- 6. the annealer -----------------------------------------------------------------------------------------------------------------------------
def lattice_model(sg):
    g, h = tg.shape("lattice6")
    n = 216
    J = np.zeros((n, n), np.float32)
    for i in range(n):
        J[i, g[1][g[0][i]:g[0][i + 1]]] = g[2][g[0][i]:g[0][i + 1]]
    model = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=True))
    model.set_couplings_from_matrix(torch.from_numpy(J))
    model.set_external_fields(torch.from_numpy(h))
    return model, n


def test_annealer_with_a_field_ladder_is_the_sequence_of_engine_calls(sg):
    model, n = lattice_model(sg)
    P, G, T, ns = 4, 3, 0.25, 6
    cfg = sg.SimulatedQuantumAnnealingConfig(n_slices=P, n_instances=G, temperature=T, n_sweeps=ns, seed=77, measure_interval=3,
                                             transverse_field=sg.TransverseField("constant", initial=1.0),
                                             field_ladder=[0.9, 1.0, 1.1], field_exchange_interval=2,
                                             worldline_clusters=True, cluster_interval=4)
    sqa = sg.SimulatedQuantumAnnealing(cfg)
    res = sqa.run(model)
    k = cfg.couplings_by_instance()
    assert k.shape == (ns, G)
    attempts, accepts = np.zeros(G - 1, np.int64), np.zeros(G - 1, np.int64)
    history = []
    with sg.AnnealEngine(0) as e:
        model.load_into(e)
        e.init_replicas(P * G, seed=77)
        e.set_temperatures(P * T)
        for t in range(ns):
            e.sweep_transverse(1, P, k[t:t + 1])
            if (t + 1) % 4 == 0:  # a cluster sweep due at that sweep runs first
                e.worldline_clusters(1, P, sg.bond_probability(k[t], P * T)[None, :], round=t)
            if (t + 1) % 2 == 0:
                parity = ((t + 1) // 2 - 1) & 1
                acc, _ = e.exchange_transverse(P, k[t], parity=parity, round=t)
                lower = np.arange(parity, G - 1, 2)
                attempts[lower] += 1
                accepts[lower] += acc[lower]
            if (t + 1) % 3 == 0:
                history.append(float(e.energies().min()))
        energies, links, best = e.energies().reshape(G, P), e.time_links(P), e.best()
    assert res.energy_history == history and res.best_energy == best[0]
    assert np.array_equal(sqa.final_energies, energies) and np.array_equal(sqa.time_links, links)
    assert np.array_equal(sqa.field_exchange_statistics[0], attempts) and np.array_equal(sqa.field_exchange_statistics[1], accepts)
    assert np.array_equal(attempts, [2, 1]) and np.array_equal(accepts, [1, 1])  # (as the references compose this chain)
    want_m = sg.transverse_magnetization(links, n, P, np.asarray([0.9, 1.0, 1.1]), T)
    assert np.array_equal(sqa.transverse_magnetization, want_m) and np.all(want_m > 0)
    q = sg.quantum_energy(sqa.final_energies, sqa.time_links, n, P, np.asarray([0.9, 1.0, 1.1]), T)
    assert q.shape == (G,) and np.all(q < sqa.final_energies.mean(axis=1))


def test_annealer_with_the_defaults_is_the_parents_sequence(sg):
    model, n = lattice_model(sg)
    P, G, T, ns = 4, 2, 0.25, 6
    cfg = sg.SimulatedQuantumAnnealingConfig(n_slices=P, n_instances=G, temperature=T, n_sweeps=ns, seed=78, measure_interval=4,
                                             transverse_field=sg.TransverseField("linear_decrease", initial=2.0, final=0.5))
    sqa = sg.SimulatedQuantumAnnealing(cfg)
    res = sqa.run(model)
    assert sqa.field_exchange_statistics is None
    k, gam = cfg.couplings(), cfg.transverse_field.gammas(ns)
    history, acc_history, acc_prev = [], [], np.zeros(P * G, np.int64)
    with sg.AnnealEngine(0) as e:
        model.load_into(e)
        e.init_replicas(P * G, seed=78)
        e.set_temperatures(P * T)
        for k0 in range(0, ns, 4):
            step = min(4, ns - k0)
            e.sweep_transverse(step, P, k[k0:k0 + step])
            en, acc, _ = e.snapshot(slots=False)
            history.append(float(en.min()))
            acc_history.append(float((acc - acc_prev).sum()) / float(P * G * n * step))
            acc_prev = acc
        energies, links, best = e.energies().reshape(G, P), e.time_links(P), e.best()
    assert res.energy_history == history and res.acceptance_rate_history == acc_history
    assert res.temperature_history == [float(gam[3]), float(gam[5])]
    assert res.best_energy == best[0] and np.array_equal(res.best_configuration.numpy().astype(np.int8), best[1])
    assert np.array_equal(sqa.final_energies, energies) and np.array_equal(sqa.time_links, links)
    assert np.array_equal(sqa.transverse_magnetization, sg.transverse_magnetization(links, n, P, float(gam[-1]), T))
