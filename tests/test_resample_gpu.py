"""Population annealing's resampling step on the engine (sga_resample, csrc/resample.hip) against the integer reference
of tests/resample_reference.py: the plan over shapes that cross every chunk of the kernels, over the inputs that decide
it, the state the call leaves, the chain that continues from it on every kind of problem, shards, batches, every
refusal, and the whole method (PopulationAnnealing.run) against the CPU loop.  Every comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
import resample_reference as rr
import stream_forms as sf
from test_resample_host import SEED, complete_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


# ----------------------------------------------------------------------------- helpers
def raw_resample(e, dbeta, P, round_, parents=True):
    """sga_resample with host outputs: (parents int32 [R], shift float64 [P], weight_sum uint64 [P]), the call's exact results."""
    from spin_glass_anneal_rl_amd import _native as N
    db = np.ascontiguousarray(np.broadcast_to(np.asarray(dbeta, np.float64), (P,)))
    par, shift, S = np.full(e.R, -7, np.int32), np.zeros(P), np.zeros(P, np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    N.check(e._lib.sga_resample(e._h, P, ptr(db), int(round_) & 0xFFFFFFFF, ptr(par) if parents else None, ptr(shift), ptr(S)),
            "sga_resample")
    return par, shift, S


def int_energy(J, h, s):
    """E = -1/2 s J s - h s of integer problems, exact in fp64."""
    s = s.astype(np.float64)
    return -(0.5 * np.einsum("ri,ij,rj->r", s, J.astype(np.float64), s) + s @ h.astype(np.float64))


def snapshot(e):
    """Everything the call may or may not touch, replica by replica (small R)."""
    best = [e.best(r) for r in range(e.R)]
    st = dict(spins=[e.spins(r) for r in range(e.R)], energy=e.energies(), best_e=np.asarray([b[0] for b in best]),
              best_s=[b[1] for b in best], acc=e.stats()[0], temps=e.temperatures(), counters=e.counters())
    if e.n_ladders > 0:
        st["slot_map"], st["exchange"] = e.slot_map(), np.stack(e.exchange_stats())
    return st


def expected(before, parents):
    """The state section 3 of the header promises: (state, destinations whose best followed, whose best was kept)."""
    after = dict(before)  # (accept counters, temperatures, counters, slot map, exchange statistics: as they were)
    after["spins"], after["best_s"] = list(before["spins"]), list(before["best_s"])
    after["energy"], after["best_e"] = before["energy"].copy(), before["best_e"].copy()
    took = kept = 0
    for d, p in enumerate(parents):
        if p == d:
            continue
        after["spins"][d] = before["spins"][p]
        after["energy"][d] = before["energy"][p]
        if before["energy"][p] < before["best_e"][d]:
            after["best_e"][d], after["best_s"][d] = before["energy"][p], before["spins"][p]
            took += 1
        else:
            kept += 1
    return after, took, kept


def assert_state(got, want, tag):
    assert list(got) == list(want), tag
    for k in want:
        if isinstance(want[k], list):
            assert len(got[k]) == len(want[k]) and all(np.array_equal(a, b) for a, b in zip(got[k], want[k])), (tag, k)
        elif isinstance(want[k], tuple):
            assert tuple(got[k]) == want[k], (tag, k)
        else:
            assert np.array_equal(got[k], want[k]), (tag, k)


def refused(fn, *a, **kw):
    from spin_glass_anneal_rl_amd.exceptions import AnnealingError
    with pytest.raises(AnnealingError) as exc:
        fn(*a, **kw)
    return str(exc.value)


# ----------------------------------------------------------------------------- the plan: shapes
@pytest.mark.parametrize("P", [1, 3, 8])
@pytest.mark.parametrize("N,n", [(1, 15), (2, 16), (3, 17), (64, 33), (65, 15), (257, 16), (1025, 17), (4097, 33)])
def test_plan_shapes(sg, N, n, P):
    """Row lengths on both sides of the 16-byte chunks, populations from one member to sixteen members a thread."""
    te = sf._te()
    R = N * P
    J, h = te.int_couplings(n, 40 + n, 3), sf._fields(n, 41 + n, -2, 2)
    s0 = (np.random.RandomState(1000 * N + P).randint(0, 2, (R, n)) * 2 - 1).astype(np.int8)
    E = int_energy(J, h, s0)
    db = np.linspace(0.04, 0.12, P)
    with sg.AnnealEngine(0) as e:
        e.set_dense(J, h)
        e.init_replicas(R, seed=SEED, s0=s0)
        assert np.array_equal(e.energies(), E)
        par, shift, S = raw_resample(e, db, P, 7)
        ref = rr.plan_all(E, db, P, SEED, 7)
        assert np.array_equal(par, ref[0]) and np.array_equal(shift, ref[1]) and np.array_equal(S, ref[2])
        assert np.array_equal(e.spins(), s0[par]) and np.array_equal(e.energies(), E[par])
        if N > 2:
            assert np.any(par != np.arange(R))  # the case copies something


# ----------------------------------------------------------------------------- the plan: inputs
N_IN, P_IN, n_IN = 65, 3, 33


@pytest.fixture(scope="module")
def inputs_problem():
    te = sf._te()
    J, h = te.int_couplings(n_IN, 5, 5), sf._fields(n_IN, 6, -3, 3)
    s0 = (np.random.RandomState(77).randint(0, 2, (N_IN * P_IN, n_IN)) * 2 - 1).astype(np.int8)
    return J, h, s0, int_energy(J, h, s0)


@pytest.mark.parametrize("case,dbeta,round_,seed", [
    ("positive", 0.05, 0, SEED), ("negative", -0.05, 0, SEED), ("zero", 0.0, 0, SEED), ("per-population", [0.08, -0.03, 0.0], 0, SEED),
    ("one-takes-all", 50.0, 0, SEED), ("weights-truncate-to-zero", 0.2, 0, SEED),
    ("round-1", 0.05, 1, SEED), ("round-2^32-1", 0.05, 2 ** 32 - 1, SEED), ("small-seed", 0.05, 0, 12345),
    ("seed-high-half-only", 0.05, 0, 0xABCD << 32)])
def test_plan_inputs(sg, inputs_problem, case, dbeta, round_, seed):
    J, h, s0, E = inputs_problem
    R = N_IN * P_IN
    ref = rr.plan_all(E, dbeta, P_IN, seed, round_)
    pops = [rr.plan(E[p * N_IN:(p + 1) * N_IN], np.broadcast_to(dbeta, (P_IN,))[p], seed, round_, p) for p in range(P_IN)]
    if case == "zero":
        assert ref[0].tolist() == list(range(R)) and np.all(ref[1] == 0.0)
    if case == "one-takes-all":
        assert all(int(pp[3].max()) == N_IN for pp in pops)
    if case == "weights-truncate-to-zero":
        W = rr.weights(E[:N_IN], dbeta)[0]
        assert W.count(0) > 5 and sum(w > 0 for w in W) > 2
    if case == "round-2^32-1":
        assert not np.array_equal(ref[0], rr.plan_all(E, dbeta, P_IN, seed, 0)[0])
    with sg.AnnealEngine(0) as e:
        e.set_dense(J, h)
        e.init_replicas(R, seed=seed, s0=s0)
        par, shift, S = raw_resample(e, dbeta, P_IN, round_)
        assert np.array_equal(par, ref[0]) and np.array_equal(shift, ref[1]) and np.array_equal(S, ref[2]), case
        assert np.array_equal(e.spins(), s0[par]) and np.array_equal(e.energies(), E[par])
        # the Python face: the same plan (the state is now E[par]), the logarithm taken on the host
        E2 = E[par]
        ref2 = rr.plan_all(E2, dbeta, P_IN, seed, round_ + 1)
        par2, log_q = e.resample(dbeta, n_populations=P_IN, round=round_ + 1)
        assert np.array_equal(par2, ref2[0]) and np.array_equal(log_q, rr.log_q(ref2[1], ref2[2], N_IN))
        assert par2.dtype == np.int32 and log_q.dtype == np.float64


def test_device_outputs_and_the_round_counter(sg, inputs_problem):
    """A CUDA tensor for parents: filled on the device, log_q a CUDA tensor; round=None: the exchange-round counter."""
    J, h, s0, E = inputs_problem
    R = N_IN * P_IN
    with sg.AnnealEngine(0) as e:
        e.set_dense(J, h)
        e.init_replicas(R, seed=SEED, s0=s0)
        e.set_counters(0, 41)
        out = torch.full((R,), -1, dtype=torch.int32, device="cuda")
        par, log_q = e.resample(0.05, n_populations=P_IN, parents=out)
        ref = rr.plan_all(E, 0.05, P_IN, SEED, 41)
        assert par is out and log_q.is_cuda
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ref[0])
        assert np.allclose(log_q.cpu().numpy(), rr.log_q(ref[1], ref[2], N_IN), rtol=1e-14, atol=0)
        assert e.counters() == (0, 41)  # no counter moved
        assert e.resample(0.0, n_populations=P_IN, parents=False)[0] is None
        for bad in (torch.zeros(R, dtype=torch.int64, device="cuda"), torch.zeros(R - 1, dtype=torch.int32, device="cuda"),
                    torch.zeros(R, dtype=torch.int32)):
            assert "parents must be" in refused(e.resample, 0.05, P_IN, parents=bad)


# ----------------------------------------------------------------------------- the state
def test_state_after_the_call(sg):
    """Spins, energies and bests of the destinations, one whose old best beats its parent among them; every survivor, the
    counters, temperatures, slot map, exchange statistics and sweep counters as they were; energies() as recomputed."""
    te, n, R, P = sf._te(), 33, 64, 2
    J, h = te.int_couplings(n, 9, 3), sf._fields(n, 10, -2, 2)
    with sg.AnnealEngine(0) as e:
        e.set_dense(J, h)
        e.init_replicas(R, seed=SEED)
        e.set_ladder(np.zeros(R), 2)
        e.sweep(2)  # T = 0: every best is a low energy
        # odd replicas go hot: their energies rise above their bests
        e.set_ladder(np.where(np.arange(R) % 2 == 1, np.inf, 0.0), 2)
        e.sweep(2)
        e.exchange()
        before = snapshot(e)
        # population 0 favours the cold replicas (a destination's best follows where the parent lies below it), population
        # 1 the hot ones (their energies lie above every destination's best: the bests are kept)
        dbeta = [0.25, -0.1]
        ref = rr.plan_all(before["energy"], dbeta, P, SEED, 5)
        par, shift, S = raw_resample(e, dbeta, P, 5)
        assert np.array_equal(par, ref[0]) and np.array_equal(shift, ref[1]) and np.array_equal(S, ref[2])
        want, took, kept = expected(before, par)
        print(f"destinations: {took + kept}, best followed: {took}, best kept: {kept}")
        assert took > 0 and kept > 0
        assert_state(snapshot(e), want, "after sga_resample")
        assert min(want["best_e"]) == min(before["best_e"])  # the best over all replicas is never lost
        after = e.energies()
        e.recompute_energies()
        assert np.array_equal(e.energies(), after)


# ----------------------------------------------------------------------------- the chain continues
def _built(name):
    if name in ("P1", "P2"):
        import engine_reuse as er
        return er.BY_ID[name].build(), 0, 0
    f = sf.BY_NAME[name]
    return f.build(), f.rule, f.site_mode


@pytest.mark.parametrize("name", ["dense-i8-look1", "clf-one-accept", "row-shared-W256-planes", "csr-upd4", "csr-force-bits",
                                  "P1", "tsp-one-update"])
def test_the_chain_continues_from_the_resampled_state(sg, name):
    """After a call a fresh engine started from the read-back spins, with the same seed and sweep counter, walks the same
    chain for 3 sweeps -- through the form's own kernels, with the cached fields seeded again where the form keeps them."""
    b, rule, site_mode = _built(name)
    prob, R, P = b.models[0], 34, 2
    temps = sf.temps_for(b, R)
    with sg.AnnealEngine(0) as e:
        b.setup(e)
        e.set_update_rule(rule)
        e.init_replicas(R, seed=SEED)
        e.set_temperatures(temps)
        e.sweep(2, site_mode=site_mode)
        if b.want is not None:
            assert b.want(e.last_kernel(), e.describe()), (name, e.last_kernel(), e.describe())
        before = snapshot(e)
        dbeta = 1.5 / max(float(np.std(before["energy"])), 1e-9)
        ref = rr.plan_all(before["energy"], dbeta, P, SEED, 2)
        par, shift, S = raw_resample(e, dbeta, P, 2)
        assert np.array_equal(par, ref[0]) and np.array_equal(shift, ref[1]) and np.array_equal(S, ref[2]), name
        assert np.count_nonzero(par != np.arange(R)) >= 4, (name, par)
        want, _, _ = expected(before, par)
        mid = snapshot(e)
        assert_state(mid, want, (name, "after sga_resample"))
        trace = e.sweep(3, site_mode=site_mode, energy_trace=True)["energy_trace"]
        if b.want is not None:
            assert b.want(e.last_kernel(), e.describe()), (name, e.last_kernel(), e.describe())
        end = snapshot(e)
    with sg.AnnealEngine(0) as f:
        b.setup(f)
        f.set_update_rule(rule)
        f.init_replicas(R, seed=SEED, s0=np.stack(mid["spins"]))
        f.set_temperatures(temps)
        f.set_counters(2, 0)
        assert np.array_equal(f.energies(), mid["energy"]), name  # the copied bits are the from-scratch energies
        trace_f = f.sweep(3, site_mode=site_mode, energy_trace=True)["energy_trace"]
        fresh = snapshot(f)
    assert np.array_equal(trace, trace_f), name
    for k in ("spins", "energy", "counters", "temps"):
        assert_state({k: end[k]}, {k: fresh[k]}, (name, k))
    assert np.array_equal(end["acc"] - mid["acc"], fresh["acc"]), name
    # ... and it is the oracle's chain
    s = np.stack(mid["spins"]).copy()
    out = oracle.sweeps(prob, s, temps, 3, site_mode=site_mode, rule=rule, seed=SEED, sweep0=2, energy=mid["energy"], n_threads=8)
    assert np.array_equal(out["energy_trace"], trace) and np.array_equal(s, np.stack(end["spins"])), name


# ----------------------------------------------------------------------------- shards
def test_two_shards_equal_one_engine(sg):
    b = sf.BY_NAME["csr-upd4"].build()
    Rg, P = 24, 4
    temps = sf.temps_for(b, Rg)

    def run(g0, R, pops):
        with sg.AnnealEngine(0) as e:
            b.setup(e)
            e.init_replicas(R, seed=SEED, R_global=Rg, replica0=g0)
            e.set_temperatures(temps[g0:g0 + R])
            e.sweep(2)
            E = e.energies()
            par, shift, S = raw_resample(e, 0.3, pops, 9)
            ref = rr.plan_all(E, 0.3, pops, SEED, 9, replica0=g0)
            assert np.array_equal(par, ref[0]) and np.array_equal(shift, ref[1]) and np.array_equal(S, ref[2]), g0
            e.sweep(1)
            return par, shift, S, e.spins(), e.energies()
    one = run(0, Rg, P)
    lo, hi = run(0, 12, 2), run(12, 12, 2)
    assert np.array_equal(one[0], np.concatenate([lo[0], hi[0] + 12]))
    for k in (1, 2, 3, 4):
        assert np.array_equal(one[k], np.concatenate([lo[k], hi[k]])), k
    assert np.any(one[0] != np.arange(Rg))


# ----------------------------------------------------------------------------- batches
def _shared_dense():
    te, n, M = sf._te(), 96, 3
    J, H = te.pm1(n, 31), np.stack([sf._fields(n, 32 + m, -2, 2) for m in range(M)])
    return sf.Built([oracle.Problem(J=J, h=H[m]) for m in range(M)], lambda e: e.set_dense_shared(J, H), None, (30.0, 1.0))


def _shared_csr():
    te, n, M = sf._te(), 200, 3
    J, H = te.sparse_int(n, 8, 2, 33), np.stack([sf._fields(n, 34 + m, -2, 2) for m in range(M)])
    csr = te.csr_of(J)
    return sf.Built([oracle.Problem(csr=csr, h=H[m]) for m in range(M)], lambda e: e.set_csr_shared(*csr, H), None, (12.0, 0.4))


@pytest.mark.parametrize("per_model", [1, 2])
@pytest.mark.parametrize("kind", ["stacked", "shared", "shared-csr", "ragged"])
def test_batches(sg, kind, per_model):
    b = {"stacked": sf.dense_batch(False), "shared": _shared_dense, "shared-csr": _shared_csr, "ragged": sf.ragged_batch}[kind]()
    M = len(b.models)
    R, P = 8 * M, per_model * M
    with sg.AnnealEngine(0) as e:
        b.setup(e)
        e.init_replicas(R, seed=SEED)
        e.set_temperatures(sf.temps_for(b, R))
        e.sweep(2)
        before = snapshot(e)
        dbeta = np.linspace(0.5, 1.5, P) / max(float(np.std(before["energy"][:8])), 1e-9)
        ref = rr.plan_all(before["energy"], dbeta, P, SEED, 3)
        par, shift, S = raw_resample(e, dbeta, P, 3)
        assert np.array_equal(par, ref[0]) and np.array_equal(shift, ref[1]) and np.array_equal(S, ref[2]), kind
        assert np.any(par != np.arange(R))
        assert_state(snapshot(e), expected(before, par)[0], (kind, P))
        after = e.energies()
        e.recompute_energies()
        assert np.array_equal(e.energies(), after), kind
        # one population over two models is refused, the state untouched
        mid = snapshot(e)
        assert "two models" in refused(raw_resample, e, 0.1, 1, 0)
        assert_state(snapshot(e), mid, (kind, "after the refusal"))


# ----------------------------------------------------------------------------- refusals
def test_refusals_leave_the_state_untouched(sg):
    """Every refusal of include/sga.h on an engine, the state compared before and after (a population across two models:
    test_batches; more than 2^23 members needs as many replicas and is held by the stand-alone check of
    tests/test_resample_host.py, which runs the same function the call runs)."""
    from spin_glass_anneal_rl_amd import _native as N
    te, n, R = sf._te(), 17, 8
    J, h = te.pm1(n, 3), sf._fields(n, 4)
    L = N.lib()
    db = np.asarray([0.5, 0.5], np.float64)
    dbp = db.ctypes.data_as(C.c_void_p)
    assert L.sga_resample(None, 1, dbp, 0, None, None, None) == N.ERR_INVALID  # a NULL engine
    with sg.AnnealEngine(0) as e:
        assert "no couplings" in refused(raw_resample, e, 0.5, 1, 0)
        e.set_dense(J, h)
        assert "no replicas" in refused(raw_resample, e, 0.5, 1, 0)
        e.init_replicas(R, seed=SEED)
        e.set_ladder(np.linspace(3.0, 0.5, R), 1)
        e.sweep(2)
        e.exchange()
        before = snapshot(e)
        assert e._lib.sga_resample(e._h, 1, None, 0, None, None, None) == N.ERR_INVALID and "NULL" in N.last_error()
        assert "at least 1" in refused(raw_resample, e, 0.5, 0, 0)
        assert "at least 1" in refused(e.resample, 0.5, n_populations=-1)
        assert "does not divide" in refused(raw_resample, e, 0.5, 3, 0)
        for bad in (np.nan, np.inf, -np.inf):
            assert "finite" in refused(raw_resample, e, bad, 1, 0)
            assert "finite" in refused(raw_resample, e, [0.5, bad], 2, 0)
            assert "finite" in refused(e.resample, bad)
        dev = torch.full((2,), 0.5, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert e._lib.sga_resample(e._h, 2, C.c_void_p(dev.data_ptr()), 0, None, None, None) == N.ERR_INVALID
        assert "host buffer" in N.last_error()
        assert "one entry per population" in refused(e.resample, [0.1, 0.2, 0.3], n_populations=2)
        assert_state(snapshot(e), before, "after the refusals")
        # ... and the engine still serves the call
        par, _, _ = raw_resample(e, 0.5, 2, 0)
        assert np.array_equal(par, rr.plan_all(before["energy"], 0.5, 2, SEED, 0)[0])
    with sg.AnnealEngine(0) as e:  # a shard whose first replica lies inside a population
        e.set_dense(J, h)
        e.init_replicas(8, seed=SEED, R_global=12, replica0=4)
        before = snapshot(e)
        assert "shard boundary" in refused(raw_resample, e, 0.5, 1, 0)
        assert_state(snapshot(e), before, "after the shard refusal")
        par, _, _ = raw_resample(e, 0.5, 2, 0)  # populations of 4: replica0 = 4 is a boundary between two
        assert np.array_equal(par, rr.plan_all(before["energy"], 0.5, 2, SEED, 0, replica0=4)[0])


# ----------------------------------------------------------------------------- the whole method
def test_population_annealing_run_equals_the_cpu_loop(sg):
    """PopulationAnnealing.run on the n = 8 complete graph of tests/test_resample_host.py equals the CPU loop bit for bit:
    the parents of every step, the final energies, log_partition -- so the physics check of the host test holds for the
    engine without a tolerance."""
    n, Np, P, steps, sps = 8, 256, 16, 10, 2
    J, h = complete_graph(n)
    model = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=False))
    model.set_couplings_from_matrix(torch.from_numpy(J))
    model.set_external_fields(torch.from_numpy(h))
    cfg = sg.PopulationAnnealingConfig(population_size=Np, n_populations=P, beta_max=1.0, n_steps=steps, sweeps_per_step=sps,
                                       random_seed=SEED)
    pa = sg.PopulationAnnealing(cfg)
    res = pa.run(model, record_parents=True)
    ref = rr.run(oracle.Problem(J=J, h=h), Np, P, cfg.schedule(), sps, SEED, n_threads=8)
    assert np.array_equal(pa.parents_history, ref["parents"])
    assert np.array_equal(pa.final_energies, ref["energy"])
    assert np.array_equal(pa.log_partition, ref["log_partition"])
    assert np.array_equal(res.energy_history, ref["mean_energy"])
    assert np.array_equal(pa.free_energy, -ref["log_partition"] / 1.0)
    assert res.algorithm == "population_annealing" and res.n_sweeps == steps * sps and res.best_energy <= ref["energy"].min()
    # the bookkeeping: families from the recorded parents
    fam = np.tile(np.arange(Np), P)
    for p in ref["parents"]:
        fam = fam[p]
    fam = fam.reshape(P, Np)
    assert np.array_equal(pa.family_counts, [np.unique(f).size for f in fam])
    assert pa.rho_t.shape == (P,) and np.all(pa.rho_t >= 1.0) and np.all(pa.family_counts >= 1)
    assert pa.survivor_fraction.shape == (steps, P) and np.all((pa.survivor_fraction > 0) & (pa.survivor_fraction <= 1))
    assert np.array_equal(pa.survivor_fraction[0], (ref["parents"][0] == np.arange(Np * P)).reshape(P, Np).mean(axis=1))
