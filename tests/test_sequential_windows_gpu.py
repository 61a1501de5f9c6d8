"""Sequential windows (sga_set_sequential_windows, csrc/sweep_dense_seq.hip): SITE_SEQUENTIAL sweeps whose window-start
fields come from one product on the matrix cores walk the oracle's strictly sequential chain bit for bit -- energy
trace, spins, accept counts, bests -- at the shapes where the product and the chain can go wrong, under every rule and
arithmetic the form serves, at T = 0 and T = inf, across exchanges, over shared couplings, on a shard and through the
public classes; what stays off the form keeps its kernel and its chain.

The oracle takes recorded uniforms in sequential order: Philox cases hand it its own stream_u as replay_u (the engine
draws them itself), the others give one numpy array to both.

describe(): the " sweep=seq-windows(W=...)" tag belongs to the engine and its problem, not to a call (sga_describe
knows no call arguments) -- so of the cases that stay off the form, the two whose PROBLEM qualifies (a random-site call,
a traced call) keep the tag and are pinned by their kernel note alone; every other one asserts the tag's absence."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

INF = float("inf")
SEQ = oracle.SITE_SEQUENTIAL
RULES = {"metropolis": oracle.RULE_METROPOLIS, "glauber": oracle.RULE_GLAUBER, "heat-bath": oracle.RULE_HEAT_BATH}


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def sym(U):
    U = np.triu(np.asarray(U, np.float32), 1)
    return U + U.T


def int_couplings(n, seed, amp, density=1.0):
    rng = np.random.RandomState(seed)
    if amp == 1 and density == 1.0:
        return sym(rng.randint(0, 2, (n, n)) * 2 - 1)
    J = sym(rng.randint(-amp, amp + 1, (n, n)) * (rng.rand(n, n) < density))
    if n > 3:  # the largest magnitude is present
        J[0, 1] = J[1, 0] = amp
    return J


def grid_couplings(n, seed, amp, k):
    """J = m 2^-k with integers |m| <= amp, both signs of the largest magnitude and an odd m present (so k is k)."""
    rng = np.random.RandomState(seed)
    m = rng.randint(0, 2, (n, n)) * 2 - 1 if amp == 1 else rng.randint(-amp, amp + 1, (n, n))
    if n > 3:
        m[0, 1], m[0, 2], m[0, 3] = amp, -amp, 1
    return sym(m) * np.float32(2.0 ** -k)


def field(n, seed, kind, unit=1.0):
    rng = np.random.RandomState(seed)
    if kind == "int":
        return rng.randint(-3, 4, n).astype(np.float32)
    if kind == "half":
        return (rng.randint(-3, 4, n) + 0.5).astype(np.float32)
    if kind == "zero":
        return np.zeros(n, np.float32)
    return (rng.randn(n) * unit).astype(np.float32)


def ladder(R, tmax, tmin):
    return np.asarray([tmax * (tmin / tmax) ** (i / max(R - 1, 1)) for i in range(R)])


def philox_u(seed, R, ns, n, replica0=0, sweep0=0):
    """update t of sweep k of replica r takes its own Philox uniform: the oracle's stream, as recorded uniforms"""
    return np.asarray([[oracle.stream_u(seed, replica0 + r, sweep0 + k, t) for k in range(ns) for t in range(n)]
                       for r in range(R)], np.float32)


def drawn_u(seed, R, ns, n):
    return np.random.RandomState(seed).rand(R, ns * n).astype(np.float32)


def check_against(e, ref, s, out, R):
    assert np.array_equal(out["energy_trace"], ref["energy_trace"])
    assert np.array_equal(e.spins(), s)
    assert np.array_equal(e.stats()[0], ref["n_accepted"])
    for r in range(R):
        be, bs, _ = e.best(r)
        assert be == ref["best_energy"][r] and np.array_equal(bs, ref["best_spins"][r])


def on_the_form(e, W, ref=None, total=None):
    k, d = e.last_kernel(), e.describe()
    assert k.startswith("sweep_dense_seq<") and f" W={W}" in k and "(sequential windows: product on " in k, k
    assert f"sweep=seq-windows(W={W})" in d, d
    if ref is not None:
        assert 0 < ref["n_accepted"].sum() < total  # both outcomes of the rule


MAIN = {
    # name: (n, R, W, storage, amp, grid k (None: the integer form), h, philox, sweeps, the product's cores)
    "n3-partial-window-partial-block": (3, 4, 256, "f32", 1, None, "int", True, 4, "i8"),
    "n257-second-window-of-one-site": (257, 1, 256, "f32", 1, None, "int", True, 4, "i8"),
    "n64-r33-replica-tile-edge": (64, 33, 256, "f32", 1, None, "int", False, 4, "i8"),
    "n1000-r130-int8-rows-two-replica-tiles": (1000, 130, 512, "i8", 100, None, "int", False, 2, "i8"),
    "n2500-converted-rows-partial-last-window": (2500, 3, 1024, "f32", 3, None, "int", False, 3, "i8"),
    "n700-f32-product": (700, 6, 256, "f32", 200, None, "int", False, 4, "f32"),
    "n900-bit-planes-half-integer-h": (900, 4, 512, "t2", 1, 0, "half", False, 4, "i8"),
    "n700-grid-quarters-real-h": (700, 3, 256, "f32", 1, 2, "randn", False, 4, "i8"),
}


def main_problem(name):
    n, R, W, storage, amp, k, hkind, philox, ns, cores = MAIN[name]
    unit = 2.0 ** -(k or 0)
    if k is None or k == 0:
        J = int_couplings(n, 5 + n, amp, density=0.6 if storage == "t2" else 1.0)
    else:
        J = grid_couplings(n, 5 + n + amp, amp, k)
    h = field(n, n + amp, hkind, unit=max(unit * amp, unit))
    seed = 2777 + n
    temps = ladder(R, 2.0 * amp * unit * np.sqrt(n), 0.3 * unit)
    u = philox_u(seed, R, ns, n) if philox else drawn_u(n, R, ns, n)
    return J, h, seed, temps, u


@pytest.mark.parametrize("name", sorted(MAIN))
def test_the_form_equals_the_oracle(sg, name):
    n, R, W, storage, amp, k, hkind, philox, ns, cores = MAIN[name]
    J, h, seed, temps, u = main_problem(name)
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(oracle.Problem(J=J, h=h), s, temps, ns, site_mode=SEQ, replay_u=u, seed=seed, n_threads=8)
    with sg.AnnealEngine(0) as e:
        e.set_option("row_shared_grid", 0 if k is None else 1)
        e.set_sequential_windows(W)
        e.set_dense(J, h, storage=storage)
        e.init_replicas(R, seed=seed)
        assert ("table_m=0 " in e.describe()) == (k is not None), e.describe()
        e.set_temperatures(temps)
        out = e.sweep(ns, site_mode=SEQ, replay_u=None if philox else u, energy_trace=True)
        on_the_form(e, W, ref, ns * n * R)
        kern = e.last_kernel()
        assert kern.startswith("sweep_dense_seq<int8_t," if storage in ("i8", "t2") else "sweep_dense_seq<float,"), kern
        assert f"product on {cores} matrix cores" in kern, kern
        assert (f"grid=2^-{k}" in kern) == (k is not None), kern
        assert "rule=" not in kern
        check_against(e, ref, s, out, R)


def rule_problem(form):
    n = 600
    if form == "integer":
        return int_couplings(n, 41, 2), field(n, 42, "int"), ladder(5, 2.0 * 2 * np.sqrt(n), 0.3)
    return grid_couplings(n, 43, 3, 2), field(n, 44, "randn", unit=0.75), ladder(5, 2.0 * 0.75 * np.sqrt(n), 0.1)


@pytest.mark.parametrize("form", ["integer", "grid"])
@pytest.mark.parametrize("how", ["metropolis-f32", "glauber", "heat-bath"])
def test_rules_and_arithmetic_equal_the_oracle(sg, how, form):
    n, R, W, ns, seed = 600, 5, 256, 4, 31337
    J, h, temps = rule_problem(form)
    rule = RULES.get(how, oracle.RULE_METROPOLIS)
    arith = oracle.ARITH_F32 if how == "metropolis-f32" else oracle.ARITH_F64
    u = drawn_u(7, R, ns, n)
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(oracle.Problem(J=J, h=h), s, temps, ns, site_mode=SEQ, arith=arith, rule=rule, replay_u=u, seed=seed,
                        n_threads=8)
    with sg.AnnealEngine(0) as e:
        e.set_option("row_shared_grid", 1 if form == "grid" else 0)
        e.set_sequential_windows(W)
        e.set_dense(J, h, storage="f32")
        e.set_update_rule(rule)
        e.init_replicas(R, seed=seed)
        e.set_temperatures(temps)
        out = e.sweep(ns, site_mode=SEQ, arith=arith, replay_u=u, energy_trace=True)
        on_the_form(e, W, ref, ns * n * R)
        assert (f", rule={how}>" in e.last_kernel()) == (how != "metropolis-f32"), e.last_kernel()
        assert ("grid=2^-2" in e.last_kernel()) == (form == "grid"), e.last_kernel()
        check_against(e, ref, s, out, R)


@pytest.mark.parametrize("tag", ["metropolis", "glauber"])
@pytest.mark.parametrize("form", ["integer", "grid"])
def test_zero_and_infinite_temperature_equal_the_oracle(sg, form, tag):
    """T = 0 and T = inf through a schedule; integer: n - 1 = 900 terms of +-1 under h = 0 give exact-zero fields
    (Metropolis: dE = +-0; Glauber: 0 / 0)."""
    R, ns, seed, W = 6, 6, 5, 512
    if form == "integer":
        n = 901
        J, h = int_couplings(n, 8, 1), field(n, 0, "zero")
        sched = np.tile(np.asarray([INF, 0.0, 40.0, 5.0, 0.0, INF]), (ns, 1))
    else:
        n = 900
        J, h = grid_couplings(n, 8, 3, 2), field(n, 9, "randn", unit=0.5)
        sched = np.tile(np.asarray([INF, 0.0, 10.0, 1.25, 0.0, INF]), (ns, 1))
    sched[3:, 2] = 0.0
    u = drawn_u(11, R, ns, n)
    s = oracle.init_spins(n, R, seed)
    if form == "integer":  # the zero fields are met
        assert (J.astype(np.int64) @ s[1].astype(np.int64) == 0).any()
    ref = oracle.sweeps(oracle.Problem(J=J, h=h), s, sched, ns, site_mode=SEQ, rule=RULES[tag], replay_u=u, seed=seed, n_threads=8)
    with sg.AnnealEngine(0) as e:
        e.set_option("row_shared_grid", 1 if form == "grid" else 0)
        e.set_sequential_windows(W)
        e.set_dense(J, h, storage="f32")
        e.set_update_rule(RULES[tag])
        e.init_replicas(R, seed=seed)
        out = e.sweep(ns, site_mode=SEQ, sched=sched, replay_u=u, energy_trace=True)
        on_the_form(e, W, ref, ns * n * R)
        check_against(e, ref, s, out, R)


def test_several_sweeps_and_exchanges_equal_the_kernel_it_replaces(sg):
    n, R, seed = 1200, 16, 99
    J, h = int_couplings(n, 3, 2), field(n, 4, "int")
    temps = ladder(R, 60.0, 0.5)
    runs = {}
    for W in (256, 0):
        with sg.AnnealEngine(0) as e:
            e.set_sequential_windows(W)
            e.set_dense(J, h, storage="f32")
            e.init_replicas(R, seed=seed)
            e.set_ladder(temps)
            trace, swaps, kernels = [], [], set()
            for _ in range(4):
                trace.append(e.sweep(3, site_mode=SEQ, energy_trace=True)["energy_trace"])
                kernels.add(e.last_kernel().split("<")[0])
                swaps.append(e.exchange())
            assert kernels == ({"sweep_dense_seq"} if W else {"sweep_dense_kernel"}), kernels
            if W:
                on_the_form(e, W)
            else:
                assert "seq-windows" not in e.describe()
            runs[W] = (np.vstack(trace), swaps, e.spins(), e.energies(), e.best()[0], e.stats()[0], e.slot_map())
    assert np.abs(np.asarray(runs[256][1])).sum() > 0  # some exchange was accepted
    assert 0 < runs[256][5].sum() < 12 * n * R
    for a, b in zip(runs[256], runs[0]):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_shared_couplings_each_model_walks_its_one_model_chain(sg):
    n, M, k, W, seed, ns = 700, 3, 2, 256, 0x5A4E, 4
    J = grid_couplings(n, 17, 3, 2)
    hs = np.stack([field(n, 1, "int"), field(n, 2, "half"), field(n, 3, "randn")]).astype(np.float32)
    temps = np.tile(ladder(k, 12.0, 0.5), M)
    u = drawn_u(13, M * k, ns, n)
    with sg.AnnealEngine(0) as e:
        e.set_option("row_shared_grid", 1)
        e.set_sequential_windows(W)
        e.set_dense_shared(J, hs)
        e.init_replicas(M * k, seed=seed)
        e.set_temperatures(temps)
        out = e.sweep(ns, site_mode=SEQ, replay_u=u, energy_trace=True)
        on_the_form(e, W)
        assert f"shared-J models={M}" in e.describe(), e.describe()
        spins, acc = e.spins(), e.stats()[0]
        bests = [e.best(r) for r in range(M * k)]
    assert 0 < acc.sum() < ns * n * M * k
    for m in range(M):
        s = oracle.init_spins(n, k, seed, replica0=m * k)
        ref = oracle.sweeps(oracle.Problem(J=J, h=hs[m]), s, temps[m * k:(m + 1) * k], ns, site_mode=SEQ, replay_u=u[m * k:(m + 1) * k],
                            seed=seed, replica0=m * k, n_threads=8)
        assert np.array_equal(out["energy_trace"][:, m * k:(m + 1) * k], ref["energy_trace"]), m
        assert np.array_equal(spins[m * k:(m + 1) * k], s), m
        assert np.array_equal(acc[m * k:(m + 1) * k], ref["n_accepted"]), m
        for r in range(k):
            assert bests[m * k + r][0] == ref["best_energy"][r] and np.array_equal(bests[m * k + r][1], ref["best_spins"][r])


def test_a_shard_walks_its_replicas_of_the_unsharded_run(sg):
    """init_replicas(R_local = 4, R_global = 12, replica0 = 5): replicas 5 ... 8 of the oracle's run, Philox uniforms"""
    n, W, seed, ns, Rg, r0, Rl = 300, 256, 606, 3, 12, 5, 4
    J, h = int_couplings(n, 51, 3), field(n, 52, "int")
    temps = ladder(Rg, 2.0 * 3 * np.sqrt(n), 0.3)
    s = oracle.init_spins(n, Rg, seed)
    ref = oracle.sweeps(oracle.Problem(J=J, h=h), s, temps, ns, site_mode=SEQ, replay_u=philox_u(seed, Rg, ns, n), seed=seed, n_threads=8)
    with sg.AnnealEngine(0) as e:
        e.set_sequential_windows(W)
        e.set_dense(J, h, storage="f32")
        e.init_replicas(Rl, seed=seed, R_global=Rg, replica0=r0)
        e.set_temperatures(temps[r0:r0 + Rl])
        out = e.sweep(ns, site_mode=SEQ, energy_trace=True)
        on_the_form(e, W)
        sl = slice(r0, r0 + Rl)
        assert 0 < ref["n_accepted"][sl].sum() < ns * n * Rl
        assert np.array_equal(out["energy_trace"], ref["energy_trace"][:, sl])
        assert np.array_equal(e.spins(), s[sl])
        assert np.array_equal(e.stats()[0], ref["n_accepted"][sl])
        for r in range(Rl):
            be, bs, _ = e.best(r)
            assert be == ref["best_energy"][r0 + r] and np.array_equal(bs, ref["best_spins"][r0 + r])


@pytest.mark.parametrize("case", ["random", "traces", "wolff", "gauss", "batch", "cache-on", "csr"])
def test_what_stays_off_the_form_walks_the_same_chain(sg, case):
    n, R, ns, seed, W = 300 if case == "wolff" else 500, 4, 3, 21, 256
    rng = np.random.RandomState(2)
    J = sym(rng.randn(n, n)) if case == "gauss" else int_couplings(n, 6, 1, density=0.05 if case == "csr" else 1.0)
    h = field(n, 7, "int")
    temps = ladder(R, 30.0, 0.5)
    prob = oracle.Problem(J=J, h=h)
    s = oracle.init_spins(n, R, seed)
    u = drawn_u(17, 2 * R, ns, n)
    with sg.AnnealEngine(0) as e:
        e.set_sequential_windows(W)
        if case == "batch":
            e.set_dense_batch(np.stack([J, J]), np.stack([h, h]), storage="f32")
            e.init_replicas(2 * R, seed=seed)
            e.set_temperatures(np.concatenate([temps, temps]))
            out = e.sweep(ns, site_mode=SEQ, replay_u=u, energy_trace=True)
            assert e.last_kernel().startswith("sweep_dense_kernel<"), e.last_kernel()
            assert "seq-windows" not in e.describe(), e.describe()
            s2 = np.concatenate([s, oracle.init_spins(n, R, seed, replica0=R)])
            for m in range(2):  # model m: the one-model problem at replica0 = m R
                part = s2[m * R:(m + 1) * R].copy()
                ref = oracle.sweeps(prob, part, temps, ns, site_mode=SEQ, replay_u=u[m * R:(m + 1) * R], seed=seed, replica0=m * R,
                                    n_threads=8)
                assert np.array_equal(out["energy_trace"][:, m * R:(m + 1) * R], ref["energy_trace"])
                assert np.array_equal(e.spins()[m * R:(m + 1) * R], part)
            return
        if case == "wolff":
            # The cluster rule: against the same run with the setting off.  One
            # Metropolis sweep comes first in both: on the form in the one, on the row kernel in the other.
            u1 = np.ascontiguousarray(u[:R, :n])
            runs = []
            for w in (W, 0):
                with sg.AnnealEngine(0) as f:
                    f.set_sequential_windows(w)
                    f.set_dense(J, h, storage="f32")
                    f.init_replicas(R, seed=seed)
                    f.set_temperatures(temps)
                    first = f.sweep(1, site_mode=SEQ, replay_u=u1, energy_trace=True)["energy_trace"]
                    assert f.last_kernel().startswith("sweep_dense_seq<" if w else "sweep_dense_kernel<"), f.last_kernel()
                    f.set_update_rule(oracle.RULE_WOLFF)
                    assert "seq-windows" not in f.describe(), f.describe()
                    out = f.sweep(ns, energy_trace=True)["energy_trace"]
                    runs.append((first, out, f.spins(), f.energies(), f.stats()[0]))
            for a, b in zip(*runs):
                assert np.array_equal(a, b)
            return
        if case == "cache-on":
            e.set_field_cache("on")
        if case == "csr":
            rowptr = np.concatenate([[0], np.cumsum((J != 0).sum(1))]).astype(np.int32)
            col = np.concatenate([np.nonzero(J[i])[0] for i in range(n)]).astype(np.int32)
            val = np.concatenate([J[i][J[i] != 0] for i in range(n)]).astype(np.float32)
            e.set_csr(rowptr, col, val, h)
        else:
            e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_temperatures(temps)
        if case == "random":
            out = e.sweep(ns, energy_trace=True)
            ref = oracle.sweeps(prob, s, temps, ns, seed=seed, n_threads=8)
        else:
            out = e.sweep(ns, site_mode=SEQ, replay_u=u[:R], energy_trace=True, trace=case == "traces")
            ref = oracle.sweeps(prob, s, temps, ns, site_mode=SEQ, replay_u=u[:R], seed=seed, n_threads=8)
        kern, d = e.last_kernel(), e.describe()
        assert not kern.startswith("sweep_dense_seq"), kern
        if case == "cache-on":
            assert "sweep=cached-local-fields" in d, d
        elif case == "csr":
            assert kern.startswith("sweep_csr"), kern
        else:
            assert kern.startswith("sweep_dense_kernel<"), kern
        # (a random-site or traced CALL on a problem that qualifies: the tag is the engine's, see the module docstring)
        assert ("seq-windows" in d) == (case in ("random", "traces")), d
        assert 0 < ref["n_accepted"].sum() < ns * n * R
        assert np.array_equal(out["energy_trace"], ref["energy_trace"])
        assert np.array_equal(e.spins(), s)
        assert np.array_equal(e.stats()[0], ref["n_accepted"])


def test_the_public_classes_return_the_result_of_the_run_without_the_windows(sg):
    from spin_glass_anneal_rl_amd.engine import last_kernel
    n = 64
    J, h = int_couplings(n, 31, 1), field(n, 32, "int")

    def model():
        m = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=False))
        m.set_couplings_from_matrix(torch.from_numpy(J))
        m.set_external_fields(torch.from_numpy(h))
        return m

    def tempering(W):
        cfg = sg.ParallelTemperingConfig(n_replicas=6, n_sweeps=30, temp_min=0.1, temp_max=3.0, exchange_interval=5, record_interval=5,
                                         random_seed=12, coupling_storage="f32", field_cache="off", autotune=False,
                                         site_order="sequential", sequential_window=W)
        pt = sg.ParallelTempering(cfg)
        res = pt.run(model())
        return (res.best_energy, res.best_configuration.numpy().copy(), np.asarray(pt.energy_histories), pt.exchange_accepts.copy(),
                last_kernel())

    def scheduler(W):
        res = sg.SpinGlassScheduler(random_seed=12).anneal(model(), n_replicas=6, n_sweeps=30, exchange_interval=5, record_interval=5,
                                                            coupling_storage="f32", field_cache="off", autotune=False,
                                                            site_order="sequential", sequential_window=W)
        return (res.best_energy, res.best_configuration.numpy().copy(), np.asarray(res.energy_history),
                np.asarray(res.acceptance_rate_history), last_kernel())

    for run in (tempering, scheduler):
        on, off = run(1024), run(0)
        assert on[4].startswith("sweep_dense_seq<float, W=1024>"), on[4]
        assert off[4].startswith("sweep_dense_kernel<"), off[4]
        for a, b in zip(on[:4], off[:4]):
            assert np.array_equal(a, b)
    with pytest.raises(sg.ConfigurationError):
        sg.SpinGlassScheduler(random_seed=1).anneal(model(), n_replicas=2, n_sweeps=1, site_order="diagonal")


def test_the_setter_validates_and_the_value_outlives_a_problem(sg):
    n = 96
    J, h = int_couplings(n, 61, 1), field(n, 62, "int")
    with sg.AnnealEngine(0) as e:
        assert e.sequential_windows() == 0
        with pytest.raises(sg.AnnealingError):
            e.set_sequential_windows(300)
        assert e.sequential_windows() == 0
        for W in (0, 256, 512, 1024):
            e.set_sequential_windows(W)
            assert e.sequential_windows() == W
        e.set_dense(J, h, storage="f32")
        assert e.sequential_windows() == 1024 and "sweep=seq-windows(W=1024)" in e.describe()
        e.set_dense(-J, h, storage="i8")
        assert e.sequential_windows() == 1024 and "sweep=seq-windows(W=1024)" in e.describe()
        e.init_replicas(3, seed=1)
        e.set_temperatures(ladder(3, 10.0, 1.0))
        e.sweep(2, site_mode=SEQ)
        assert e.last_kernel().startswith("sweep_dense_seq<int8_t, W=1024>"), e.last_kernel()
        e.set_sequential_windows(0)
        assert "seq-windows" not in e.describe()
        e.sweep(1, site_mode=SEQ)
        assert e.last_kernel().startswith("sweep_dense_kernel<"), e.last_kernel()
