"""Row-shared windows (csrc/sweep_dense_rs.hip, ANYRULE) under the Glauber and heat-bath rules: the integer form and
the grid form (option "row_shared_grid") walk the oracle's strictly sequential chain bit for bit -- energy trace, spins,
accept counts, bests -- at T = 0 and T = inf, across exchanges, over shared couplings, through the autotuner (whose pick
belongs to the rule it was timed under) and the public class; the Wolff rule, traced sweeps, Gaussian J and stacked
batches stay on the kernels they had, and Metropolis strings name no rule."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

INF = float("inf")
RULES = {"glauber": oracle.RULE_GLAUBER, "heat-bath": oracle.RULE_HEAT_BATH}  # the tag of kernel note and describe line


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
    if n > 3:  # the largest magnitude is present: the plane count is amp's
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
    if kind == "quarter":
        return (rng.randint(-6, 7, n) * 0.25).astype(np.float32)
    if kind == "half":
        return (rng.randint(-3, 4, n) + 0.5).astype(np.float32)
    return (rng.randn(n) * unit).astype(np.float32)


def ladder(R, tmax, tmin):
    return np.asarray([tmax * (tmin / tmax) ** (i / max(R - 1, 1)) for i in range(R)])


def forced(e, W=0, grid=0, on=1):
    e.set_option("row_shared", on)
    e.set_option("row_shared_grid", grid)
    e.set_option("row_shared_window", W)


def check_against(e, ref, s, out, R):
    assert np.array_equal(out["energy_trace"], ref["energy_trace"])
    assert np.array_equal(e.spins(), s)
    assert np.array_equal(e.stats()[0], ref["n_accepted"])
    for r in range(R):
        be, bs, _ = e.best(r)
        assert be == ref["best_energy"][r] and np.array_equal(bs, ref["best_spins"][r])


def on_the_form(e, tag, W):
    """kernel note and describe line name the windows and the rule"""
    k, d = e.last_kernel(), e.describe()
    assert k.startswith("sweep_dense_rs<") and f" W={W}" in k and f", rule={tag}>" in k, k
    assert f"sweep=row-shared(W={W} " in d and f" rule={tag})" in d, d


MAIN = {
    # name: (n, R, storage, amp, grid k (None: the integer form), W, h)
    "int-n3-every-site-repeats": (3, 4, "f32", 1, None, 256, "int"),
    "int-n64-partial-window-sparse": (64, 8, "f32", 1, None, 1024, "int"),
    "int-n300-one-replica-3-planes": (300, 1, "f32", 5, None, 256, "int"),
    "int-n1000-8-planes": (1000, 6, "f32", 100, None, 256, "int"),
    "int-n2500-partial-last-window": (2500, 3, "f32", 3, None, 512, "int"),
    "int-n1500-int8-on-chip": (1500, 2, "i8", 100, None, 256, "int"),
    # (half-integer h has no accept table, table_m = 0: the windows take integer J beside it as the grid 2^-0)
    "int-n900-bit-planes-half-integer-h": (900, 4, "t2", 1, 0, 512, "half"),
    "grid-n700-quarters-real-h": (700, 3, "f32", 1, 2, 256, "randn"),
    "grid-n1000-eighths-8-planes": (1000, 6, "f32", 100, 3, 256, "randn"),
    "grid-n1500-int8-rows-randn-h": (1500, 2, "i8", 5, 0, 256, "randn"),
}


@pytest.mark.parametrize("tag", sorted(RULES))
@pytest.mark.parametrize("name", sorted(MAIN))
def test_the_form_equals_the_oracle(sg, name, tag):
    n, R, storage, amp, k, W, hkind = MAIN[name]
    unit = 2.0 ** -(k or 0)
    if k is None or k == 0:
        J = int_couplings(n, 5 + n, amp, density=0.6 if storage == "t2" else 0.7 if n == 64 else 1.0)
    else:
        J = grid_couplings(n, 5 + n + amp, amp, k)
    h = field(n, n + amp, hkind, unit=max(unit * amp, unit))
    prob = oracle.Problem(J=J, h=h)
    ns, seed = 4, 2777 + n
    temps = ladder(R, 2.0 * amp * unit * np.sqrt(n), 0.3 * unit)
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(prob, s, temps, ns, rule=RULES[tag], seed=seed, n_threads=8)
    assert 0 < ref["n_accepted"].sum() < ns * n * R  # both outcomes of the rule
    with sg.AnnealEngine(0) as e:
        forced(e, W, grid=0 if k is None else 1)
        e.set_dense(J, h, storage=storage)
        e.set_update_rule(RULES[tag])
        e.init_replicas(R, seed=seed)
        assert ("table_m=0 " in e.describe()) == (k is not None), e.describe()
        e.set_temperatures(temps)
        out = e.sweep(ns, energy_trace=True)
        on_the_form(e, tag, W)
        assert (f"grid=2^-{k}," in e.last_kernel()) == (k is not None), e.last_kernel()
        if storage == "i8" and amp == 100:
            assert "on-chip conversion" in e.last_kernel(), e.last_kernel()
        check_against(e, ref, s, out, R)


@pytest.mark.parametrize("tag", sorted(RULES))
@pytest.mark.parametrize("form", ["integer", "grid"])
def test_zero_and_infinite_temperature_equal_the_oracle(sg, form, tag):
    """x = -+inf at T = 0, NaN at 0 / 0 (integer: n - 1 = 900 terms of +-1 under h = 0 give exact-zero fields) and -+0
    at T = inf, through the chain's decision."""
    R, ns, seed = 6, 6, 5
    if form == "integer":
        n = 901
        J, h = int_couplings(n, 8, 1), np.zeros(n, np.float32)
        sched = np.tile(np.asarray([INF, 0.0, 40.0, 5.0, 0.0, INF]), (ns, 1))
    else:
        n = 900
        J, h = grid_couplings(n, 8, 3, 2), field(n, 9, "randn", unit=0.5)
        sched = np.tile(np.asarray([INF, 0.0, 10.0, 1.25, 0.0, INF]), (ns, 1))
    sched[3:, 2] = 0.0
    s = oracle.init_spins(n, R, seed)
    if form == "integer":  # the zero fields are met
        assert (J.astype(np.int64) @ s[1].astype(np.int64) == 0).any()
    ref = oracle.sweeps(oracle.Problem(J=J, h=h), s, sched, ns, rule=RULES[tag], seed=seed, n_threads=8)
    assert 0 < ref["n_accepted"].sum() < ns * n * R
    with sg.AnnealEngine(0) as e:
        forced(e, 512, grid=form == "grid")
        e.set_dense(J, h, storage="f32")
        e.set_update_rule(RULES[tag])
        e.init_replicas(R, seed=seed)
        out = e.sweep(ns, sched=sched, energy_trace=True)
        on_the_form(e, tag, 512)
        check_against(e, ref, s, out, R)


@pytest.mark.parametrize("tag", sorted(RULES))
def test_several_sweeps_and_exchanges_equal_the_kernel_it_replaces(sg, tag):
    n, R, seed = 1200, 16, 99
    J, h = int_couplings(n, 3, 2), field(n, 4, "int")
    temps = ladder(R, 60.0, 0.5)
    runs = {}
    for on in (1, 0):
        with sg.AnnealEngine(0) as e:
            forced(e, 256, on=on)
            e.set_dense(J, h, storage="f32")
            e.set_update_rule(RULES[tag])
            e.init_replicas(R, seed=seed)
            e.set_ladder(temps)
            trace, swaps, kernels = [], [], set()
            for _ in range(4):
                trace.append(e.sweep(3, energy_trace=True)["energy_trace"])
                kernels.add(e.last_kernel().split("<")[0])
                swaps.append(e.exchange())
            assert kernels == ({"sweep_dense_rs"} if on else {"sweep_dense_kernel"}), kernels
            if on:
                on_the_form(e, tag, 256)
            else:
                assert "sweep=row-shared" not in e.describe()
            runs[on] = (np.vstack(trace), swaps, e.spins(), e.energies(), e.best()[0], e.stats()[0], e.slot_map())
    assert np.abs(np.asarray(runs[1][1])).sum() > 0  # some exchange was accepted
    for a, b in zip(runs[1], runs[0]):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_shared_couplings_each_model_walks_its_one_model_chain(sg):
    n, M, k, W, seed, ns = 700, 3, 2, 256, 0x5A4E, 4
    J = grid_couplings(n, 17, 3, 2)
    hs = np.stack([field(n, 1, "int"), field(n, 2, "half"), field(n, 3, "randn")]).astype(np.float32)
    temps = np.tile(ladder(k, 12.0, 0.5), M)
    with sg.AnnealEngine(0) as e:
        forced(e, W, grid=1)
        e.set_dense_shared(J, hs)
        e.set_update_rule(oracle.RULE_GLAUBER)
        e.init_replicas(M * k, seed=seed)
        e.set_temperatures(temps)
        out = e.sweep(ns, energy_trace=True)
        on_the_form(e, "glauber", W)
        assert f"shared-J models={M}" in e.describe(), e.describe()
        spins, acc = e.spins(), e.stats()[0]
        bests = [e.best(r) for r in range(M * k)]
    for m in range(M):
        s = oracle.init_spins(n, k, seed, replica0=m * k)
        ref = oracle.sweeps(oracle.Problem(J=J, h=hs[m]), s, temps[m * k:(m + 1) * k], ns, rule=oracle.RULE_GLAUBER, seed=seed,
                            replica0=m * k, n_threads=8)
        assert np.array_equal(out["energy_trace"][:, m * k:(m + 1) * k], ref["energy_trace"]), m
        assert np.array_equal(spins[m * k:(m + 1) * k], s), m
        assert np.array_equal(acc[m * k:(m + 1) * k], ref["n_accepted"]), m
        for r in range(k):
            assert bests[m * k + r][0] == ref["best_energy"][r] and np.array_equal(bests[m * k + r][1], ref["best_spins"][r])


@pytest.mark.parametrize("case", ["wolff", "traces", "gauss", "batch"])
def test_what_stays_off_the_form_walks_the_oracles_chain(sg, case):
    n, R, ns, seed = 300 if case == "wolff" else 500, 4, 3, 21  # (a cluster move costs up to n rows)
    rng = np.random.RandomState(2)
    J = sym(rng.randn(n, n)) if case == "gauss" else int_couplings(n, 6, 1)
    h = field(n, 7, "int")
    temps = ladder(R, 30.0, 0.5)
    s = oracle.init_spins(n, R, seed)
    rule = oracle.RULE_WOLFF if case == "wolff" else oracle.RULE_GLAUBER
    with sg.AnnealEngine(0) as e:
        forced(e, 256)
        if case == "batch":
            e.set_dense_batch(np.stack([J, J]), np.stack([h, h]), storage="f32")
            e.set_update_rule(rule)
            e.init_replicas(2 * R, seed=seed)
            e.set_temperatures(np.concatenate([temps, temps]))
            out = e.sweep(ns, energy_trace=True)
            assert e.last_kernel().startswith("sweep_dense_kernel<"), e.last_kernel()
            assert "sweep=row-shared" not in e.describe()
            s2 = np.concatenate([s, oracle.init_spins(n, R, seed, replica0=R)])
            for m in range(2):  # model m: the one-model problem at replica0 = m R
                part = s2[m * R:(m + 1) * R].copy()
                ref = oracle.sweeps(oracle.Problem(J=J, h=h), part, temps, ns, rule=rule, seed=seed, replica0=m * R, n_threads=8)
                assert np.array_equal(out["energy_trace"][:, m * R:(m + 1) * R], ref["energy_trace"])
                assert np.array_equal(e.spins()[m * R:(m + 1) * R], part)
            return
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_temperatures(temps)
        if case == "wolff":
            # The cluster kernel leaves no note of its own: the engine's note is that of the launch before it on this
            # thread.  One Glauber sweep with the windows off puts the row kernel's there; a Wolff sweep through the
            # windows' launcher would replace it.  (The oracle walks the same two steps.)
            e.set_update_rule(oracle.RULE_GLAUBER)
            e.set_option("row_shared", 0)
            first = e.sweep(1, energy_trace=True)
            assert e.last_kernel().startswith("sweep_dense_kernel<"), e.last_kernel()
            ref0 = oracle.sweeps(oracle.Problem(J=J, h=h), s, temps, 1, rule=oracle.RULE_GLAUBER, seed=seed, n_threads=8)
            assert np.array_equal(first["energy_trace"], ref0["energy_trace"])
            e.set_option("row_shared", 1)
            e.set_update_rule(rule)
            out = e.sweep(ns, energy_trace=True)
            ref = oracle.sweeps(oracle.Problem(J=J, h=h), s, temps, ns, rule=rule, seed=seed, sweep0=1, energy=ref0["energy"],
                                recompute_energy=True, n_threads=8)
            acc = ref0["n_accepted"] + ref["n_accepted"]
        else:
            e.set_update_rule(rule)
            out = e.sweep(ns, energy_trace=True, trace=case == "traces")
            ref = oracle.sweeps(oracle.Problem(J=J, h=h), s, temps, ns, rule=rule, seed=seed, n_threads=8)
            acc = ref["n_accepted"]
        assert e.last_kernel().startswith("sweep_dense_kernel<"), e.last_kernel()
        if case != "traces":
            assert "sweep=row-shared" not in e.describe(), e.describe()
        assert np.array_equal(out["energy_trace"], ref["energy_trace"])
        assert np.array_equal(e.spins(), s)
        assert np.array_equal(e.stats()[0], acc)


def test_metropolis_strings_name_no_rule(sg):
    n, R, seed = 500, 4, 3
    J, h = int_couplings(n, 6, 1), field(n, 7, "int")
    with sg.AnnealEngine(0) as e:
        forced(e, 256)
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_temperatures(ladder(R, 30.0, 0.5))
        e.sweep(2)
        assert e.last_kernel().startswith("sweep_dense_rs<float, planes=1, W=256> ("), e.last_kernel()
        assert "sweep=row-shared(W=256 planes=1)" in e.describe(), e.describe()
        assert "rule=" not in e.last_kernel() and "rule=" not in e.describe()


def test_the_autotuners_pick_belongs_to_its_rule(sg):
    """Option "row_shared" = 2: sga_autotune times the windows under the engine's rule, and its pick is in force only
    while that rule is.  Which way the pick goes is a measurement: not asserted."""
    n, R, seed = 2000, 64, 4242
    J, h = int_couplings(n, 11, 1), field(n, 1, "int")
    temps = ladder(R, 10.0, 0.1)
    prob = oracle.Problem(J=J, h=h)
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(prob, s, temps, 5, rule=oracle.RULE_GLAUBER, seed=seed, n_threads=16)
    with sg.AnnealEngine(0) as e:
        e.set_option("row_shared", 2)
        e.set_dense(J, h, storage="f32")
        e.set_update_rule(oracle.RULE_GLAUBER)
        e.init_replicas(R, seed=seed)
        e.set_ladder(temps)
        a = e.sweep(2, energy_trace=True)
        assert e.last_kernel().startswith("sweep_dense_kernel<")  # (nothing is tuned yet)
        before = (e.spins(), e.energies(), e.best()[0], e.stats()[0], e.counters())
        e.autotune()
        after = (e.spins(), e.energies(), e.best()[0], e.stats()[0], e.counters())
        for x, y in zip(before, after):
            assert np.array_equal(np.asarray(x), np.asarray(y))
        forms = {key for key in e.autotune_table(forms=True) if key.startswith("row-shared:")}
        assert forms == {"row-shared:W256", "row-shared:W512", "row-shared:W1024"}, forms
        b = e.sweep(3, energy_trace=True)
        picked = "sweep=row-shared(W=" in e.describe()
        assert e.last_kernel().startswith("sweep_dense_rs<float, planes=1, W=" if picked else "sweep_dense_kernel<"), e.last_kernel()
        assert not picked or (", rule=glauber>" in e.last_kernel() and " rule=glauber)" in e.describe())
        assert np.array_equal(np.concatenate([a["energy_trace"], b["energy_trace"]]), ref["energy_trace"])
        assert np.array_equal(e.spins(), s)
        assert np.array_equal(e.stats()[0], ref["n_accepted"])
        for r in range(R):
            be, bs, _ = e.best(r)
            assert be == ref["best_energy"][r] and np.array_equal(bs, ref["best_spins"][r])
        assert e.counters()[0] == 5
        # the pick was Glauber's: Metropolis runs the row-per-proposal kernel ...
        e.set_update_rule(oracle.RULE_METROPOLIS)
        assert "sweep=row-shared" not in e.describe(), e.describe()
        c = e.sweep(1, energy_trace=True)
        assert e.last_kernel().startswith("sweep_dense_kernel<"), e.last_kernel()
        ref1 = oracle.sweeps(prob, s, temps, 1, seed=seed, sweep0=5, energy=ref["energy"], n_threads=16)
        assert np.array_equal(c["energy_trace"], ref1["energy_trace"]) and np.array_equal(e.spins(), s)
        # ... and back under Glauber the pick is in force again, if it was taken
        e.set_update_rule(oracle.RULE_GLAUBER)
        assert ("sweep=row-shared(W=" in e.describe()) == picked
        d = e.sweep(1, energy_trace=True)
        assert e.last_kernel().startswith("sweep_dense_rs<float, planes=1, W=" if picked else "sweep_dense_kernel<"), e.last_kernel()
        ref2 = oracle.sweeps(prob, s, temps, 1, rule=oracle.RULE_GLAUBER, seed=seed, sweep0=6, energy=ref1["energy"], n_threads=16)
        assert np.array_equal(d["energy_trace"], ref2["energy_trace"]) and np.array_equal(e.spins(), s)


def test_the_public_class_returns_the_result_of_the_run_without_the_windows(sg, monkeypatch):
    """ParallelTempering.run(model, update_rule=UpdateRule.GLAUBER): the environment's default for "row_shared" (read
    once per engine, at its creation) decides the kernel, the result is the same from either."""
    from spin_glass_anneal_rl_amd.engine import last_kernel
    n = 64
    J, h = int_couplings(n, 31, 1), field(n, 32, "int")

    def run(on):
        monkeypatch.setenv("SGA_ROW_SHARED", "1" if on else "0")
        m = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=False))
        m.set_couplings_from_matrix(torch.from_numpy(J))
        m.set_external_fields(torch.from_numpy(h))
        cfg = sg.ParallelTemperingConfig(n_replicas=6, n_sweeps=30, temp_min=0.1, temp_max=3.0, exchange_interval=5, record_interval=5,
                                         random_seed=12, coupling_storage="f32", field_cache="off", autotune=False)
        pt = sg.ParallelTempering(cfg)
        res = pt.run(m, update_rule=sg.UpdateRule.GLAUBER)
        return (res.best_energy, res.best_configuration.numpy().copy(), np.asarray(pt.energy_histories), pt.exchange_accepts.copy(),
                last_kernel())

    on, off = run(True), run(False)
    assert on[4].startswith("sweep_dense_rs<float, planes=1, W=1024, rule=glauber>"), on[4]
    assert off[4].startswith("sweep_dense_kernel<"), off[4]
    for a, b in zip(on[:4], off[:4]):
        assert np.array_equal(a, b)
