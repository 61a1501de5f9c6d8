"""Row-shared windows on a binary grid (csrc/sweep_dense_rs.hip, GRID; option "row_shared_grid"): the dense problems
the integer form of the windows does not take -- J on a grid 2^-k under any finite h -- walk the oracle's strictly
sequential chain bit for bit: energy trace, spins, accept counts, bests.  Every plane count, both chains (decoded from
one magnitude plane, gathered from the rows of J), resident planes and the on-chip conversion, int8 and bit-plane
storage, T = 0 and T = inf, exchanges, shared couplings, the autotuner and the config flag; the problems the verdict
refuses fall back to the row-per-proposal kernel, and nothing changes while the option is at its default."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

INF = float("inf")


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def sym(U):
    U = np.triu(np.asarray(U, np.float32), 1)
    return U + U.T


def grid_couplings(n, seed, amp, k):
    """J = m 2^-k with integers |m| <= amp, both signs of the largest magnitude and an odd m present (so k is k)."""
    rng = np.random.RandomState(seed)
    m = rng.randint(0, 2, (n, n)) * 2 - 1 if amp == 1 else rng.randint(-amp, amp + 1, (n, n))
    if n > 3:
        m[0, 1], m[0, 2], m[0, 3] = amp, -amp, 1
    return sym(m) * np.float32(2.0 ** -k)


def field(n, seed, kind, unit=1.0):
    rng = np.random.RandomState(seed)
    if kind == "quarter":
        return (rng.randint(-6, 7, n) * 0.25).astype(np.float32)
    if kind == "half":
        return (rng.randint(-3, 4, n) + 0.5).astype(np.float32)
    return (rng.randn(n) * unit).astype(np.float32)


def ladder(R, tmax, tmin):
    return np.asarray([tmax * (tmin / tmax) ** (i / max(R - 1, 1)) for i in range(R)])


def forced(e, W=0, grid=1, on=1):
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


MAIN = {
    # name: (n, R, storage, amp, k, W, h, kernel's element type, planes, fields from)
    "n3-every-site-repeats": (3, 4, "f32", 1, 2, 256, "quarter", "float", 1, "resident"),
    "n64-bit-chain-unit-quarter": (64, 8, "f32", 1, 2, 1024, "randn", "float", 1, "resident"),
    "n300-one-replica-halves": (300, 1, "f32", 5, 1, 256, "quarter", "float", 3, "resident"),
    "n1000-eighths-8-planes": (1000, 6, "f32", 100, 3, 256, "randn", "float", 8, "resident"),
    "n2500-quarters-partial-window": (2500, 3, "f32", 3, 2, 512, "quarter", "float", 3, "resident"),
    "n700-grid-2^-20": (700, 3, "f32", 1, 20, 256, "grid", "float", 1, "resident"),
    "n1500-int8-rows-randn-h": (1500, 2, "i8", 5, 0, 256, "randn", "int8_t", 3, "resident"),
    "n1500-int8-rows-on-chip": (1500, 2, "i8", 100, 0, 256, "quarter", "int8_t", 8, "on-chip"),
    "n900-bit-planes-half-integer-h": (900, 4, "t2", 1, 0, 512, "half", "int8_t", 1, "resident"),
}


@pytest.mark.parametrize("name", sorted(MAIN))
def test_grid_form_equals_the_oracle(sg, name):
    from spin_glass_anneal_rl_amd.engine import last_kernel
    n, R, storage, amp, k, W, hkind, elem, planes, source = MAIN[name]
    unit = 2.0 ** -k
    J = grid_couplings(n, 5 + n + amp, amp, k)
    if name.startswith("n64"):  # J in {0, +-1/4}
        J = J * sym(np.random.RandomState(2).rand(n, n) < 0.7)
    if hkind == "grid":  # h = 2^-20 x integers
        h = (np.random.RandomState(n).randint(-3, 4, n) * unit).astype(np.float32)
    else:
        h = field(n, n + amp, hkind, unit=1.0 if hkind == "half" else max(unit * amp, unit))
    assert not np.all(h == np.rint(h)) or k > 0  # not an integer problem: the integer form does not take it
    prob = oracle.Problem(J=J, h=h)
    ns, seed = 4, 1777 + n
    temps = ladder(R, 2.0 * amp * unit * np.sqrt(n), 0.3 * unit)
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(prob, s, temps, ns, seed=seed, n_threads=8)
    assert 0 < ref["n_accepted"].sum() < ns * n * R  # both branches of the rule
    with sg.AnnealEngine(0) as e:
        forced(e, W)
        e.set_dense(J, h, storage=storage)
        e.init_replicas(R, seed=seed)
        assert "table_m=0 " in e.describe(), e.describe()
        assert f"sweep=row-shared(W={W} planes={planes} grid=2^-{k})" in e.describe(), e.describe()
        assert e.route_query().rs_grid == 1 + k
        e.set_temperatures(temps)
        out = e.sweep(ns, energy_trace=True)
        want = f"sweep_dense_rs<{elem}, planes={planes}, W={W}, grid=2^-{k}>"
        assert last_kernel().startswith(want), last_kernel()
        assert ("resident bit-planes" if source == "resident" else "on-chip conversion") in last_kernel(), last_kernel()
        check_against(e, ref, s, out, R)


def quarter_problem(n, seed, amp=3, hkind="randn"):
    return grid_couplings(n, seed, amp, 2), field(n, seed + 1, hkind, unit=0.5)


def test_zero_and_infinite_temperature_equal_the_oracle(sg):
    from spin_glass_anneal_rl_amd.engine import last_kernel
    n, R, ns, seed = 900, 6, 6, 5
    J, h = quarter_problem(n, 8)
    sched = np.tile(np.asarray([INF, 0.0, 10.0, 1.25, 0.0, INF]), (ns, 1))
    sched[3:, 2] = 0.0
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(oracle.Problem(J=J, h=h), s, sched, ns, seed=seed, n_threads=8)
    with sg.AnnealEngine(0) as e:
        forced(e, 512)
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        out = e.sweep(ns, sched=sched, energy_trace=True)
        assert last_kernel().startswith("sweep_dense_rs<float, planes=3, W=512, grid=2^-2>"), last_kernel()
        check_against(e, ref, s, out, R)
    acc = ref["n_accepted"]
    assert acc[0] == acc[5] == ns * n  # T = inf accepts every proposal


def test_several_sweeps_and_exchanges_equal_the_kernel_it_replaces(sg):
    n, R, seed = 1200, 16, 99
    J, h = quarter_problem(n, 3, amp=2, hkind="quarter")
    temps = ladder(R, 15.0, 0.125)
    runs = {}
    for grid in (1, 0):
        with sg.AnnealEngine(0) as e:
            forced(e, 256, grid=grid)
            e.set_dense(J, h, storage="f32")
            e.init_replicas(R, seed=seed)
            e.set_ladder(temps)
            trace, swaps, kernels = [], [], set()
            for _ in range(4):
                trace.append(e.sweep(3, energy_trace=True)["energy_trace"])
                kernels.add(e.last_kernel().split("<")[0])
                swaps.append(e.exchange())
            assert kernels == ({"sweep_dense_rs"} if grid else {"sweep_dense_kernel"}), kernels
            assert ("sweep=row-shared" in e.describe()) == bool(grid)
            runs[grid] = (np.vstack(trace), swaps, e.spins(), e.energies(), e.best()[0], e.stats()[0], e.slot_map())
    assert np.abs(np.asarray(runs[1][1])).sum() > 0  # some exchange was accepted
    for a, b in zip(runs[1], runs[0]):
        assert np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("case", ["gauss", "large_J", "bound", "asymmetric", "traces", "batch"])
def test_problems_the_verdict_refuses_fall_back_with_the_oracles_chain(sg, case):
    from spin_glass_anneal_rl_amd.engine import last_kernel
    n, R, ns, seed = 500, 4, 3, 21
    rng = np.random.RandomState(2)
    J, h = quarter_problem(n, 6, amp=1, hkind="quarter")
    if case == "gauss":
        J = sym(rng.randn(n, n))
    elif case == "large_J":  # 4 |J| = 300
        J = grid_couplings(n, 6, 300, 2)
    elif case == "bound":  # 2^6 x 3 10^5 > 2^24
        J, h = grid_couplings(n, 6, 1, 6), np.full(n, 3.0e5, np.float32)
    elif case == "asymmetric":
        J = J.copy()
        J[0, 1] = -J[1, 0]
    tmax = {"large_J": 2000.0, "bound": 6.0e5}.get(case, 12.0)
    temps = ladder(R, tmax, tmax / 40.0)
    s = oracle.init_spins(n, R, seed)
    with sg.AnnealEngine(0) as e:
        forced(e, 256)
        if case == "batch":
            e.set_dense_batch(np.stack([J, J]), np.stack([h, h]), storage="f32")
            e.init_replicas(2 * R, seed=seed)
            e.set_temperatures(np.concatenate([temps, temps]))
            out = e.sweep(ns, energy_trace=True)
            assert last_kernel().startswith("sweep_dense_kernel<"), last_kernel()
            assert "sweep=row-shared" not in e.describe()
            s2 = np.concatenate([s, oracle.init_spins(n, R, seed, replica0=R)])
            for m in range(2):  # model m: the one-model problem at replica0 = m R
                part = s2[m * R:(m + 1) * R].copy()
                ref = oracle.sweeps(oracle.Problem(J=J, h=h), part, temps, ns, seed=seed, replica0=m * R, n_threads=8)
                assert np.array_equal(out["energy_trace"][:, m * R:(m + 1) * R], ref["energy_trace"])
                assert np.array_equal(e.spins()[m * R:(m + 1) * R], part)
            return
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_temperatures(temps)
        assert (e.route_query().rs_grid == 0) == (case != "traces")
        out = e.sweep(ns, energy_trace=True, trace=case == "traces")
        assert last_kernel().startswith("sweep_dense_kernel<"), last_kernel()
        if case != "traces":
            assert "sweep=row-shared" not in e.describe()
        ref = oracle.sweeps(oracle.Problem(J=J, h=h), s, temps, ns, seed=seed, n_threads=8,
                            recompute_energy=case == "asymmetric")  # (asymmetric J: energies recomputed per sweep)
        assert np.array_equal(out["energy_trace"], ref["energy_trace"])
        assert np.array_equal(e.spins(), s)
        assert np.array_equal(e.stats()[0], ref["n_accepted"])


def test_the_default_leaves_a_quarter_valued_problem_on_the_row_kernel(sg):
    from spin_glass_anneal_rl_amd.engine import last_kernel
    n, R, seed = 500, 4, 3
    J, h = quarter_problem(n, 4, hkind="quarter")
    with sg.AnnealEngine(0) as e:
        e.set_option("row_shared", 1)
        assert e.get_option("row_shared_grid") == 0
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_temperatures(ladder(R, 10.0, 0.5))
        e.sweep(2)
        assert last_kernel().startswith("sweep_dense_kernel<"), last_kernel()
        assert "sweep=row-shared" not in e.describe() and "row-shared" not in e.explain_route()
        assert e.route_query().rs_grid == 3  # the verdict is kept whatever the option says


def test_shared_couplings_each_model_walks_its_one_model_chain(sg):
    n, M, k, W, seed, ns = 700, 3, 2, 256, 0x5A4E, 4
    J = grid_couplings(n, 17, 3, 2)
    hs = np.stack([field(n, 1, "half") - 0.5, field(n, 2, "quarter"), field(n, 3, "randn")]).astype(np.float32)
    assert np.all(hs[0] == np.rint(hs[0])) and not np.all(hs[1] == np.rint(hs[1]))
    temps = np.tile(ladder(k, 12.0, 0.5), M)
    with sg.AnnealEngine(0) as e:
        forced(e, W)
        e.set_dense_shared(J, hs)
        e.init_replicas(M * k, seed=seed)
        e.set_temperatures(temps)
        out = e.sweep(ns, energy_trace=True)
        assert e.last_kernel().startswith(f"sweep_dense_rs<float, planes=3, W={W}, grid=2^-2>"), e.last_kernel()
        assert f"shared-J models={M}" in e.describe() and f"sweep=row-shared(W={W} planes=3 grid=2^-2)" in e.describe(), e.describe()
        spins, acc = e.spins(), e.stats()[0]
        bests = [e.best(r) for r in range(M * k)]
    for m in range(M):
        s = oracle.init_spins(n, k, seed, replica0=m * k)
        ref = oracle.sweeps(oracle.Problem(J=J, h=hs[m]), s, temps[m * k:(m + 1) * k], ns, seed=seed, replica0=m * k, n_threads=8)
        assert np.array_equal(out["energy_trace"][:, m * k:(m + 1) * k], ref["energy_trace"]), m
        assert np.array_equal(spins[m * k:(m + 1) * k], s), m
        assert np.array_equal(acc[m * k:(m + 1) * k], ref["n_accepted"]), m
        for r in range(k):
            assert bests[m * k + r][0] == ref["best_energy"][r] and np.array_equal(bests[m * k + r][1], ref["best_spins"][r])


def test_autotune_times_the_grid_form_and_keeps_state_and_chain(sg):
    n, R, seed = 2000, 64, 4242
    J, h = quarter_problem(n, 11, amp=1, hkind="randn")
    temps = ladder(R, 2.5, 0.025)
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(oracle.Problem(J=J, h=h), s, temps, 5, seed=seed, n_threads=16)
    with sg.AnnealEngine(0) as e:
        e.set_option("row_shared", 2)
        e.set_option("row_shared_grid", 1)
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_ladder(temps)
        a = e.sweep(2, energy_trace=True)
        assert e.last_kernel().startswith("sweep_dense_kernel<")  # (option "row_shared" = 2: not before the autotuner)
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
        assert not picked or "grid=2^-2>" in e.last_kernel()
        assert np.array_equal(np.concatenate([a["energy_trace"], b["energy_trace"]]), ref["energy_trace"])
        assert np.array_equal(e.spins(), s)
        assert np.array_equal(e.stats()[0], ref["n_accepted"])
        for r in range(R):
            be, bs, _ = e.best(r)
            assert be == ref["best_energy"][r] and np.array_equal(bs, ref["best_spins"][r])


def test_config_flag_returns_the_result_of_the_run_without_it(sg, monkeypatch):
    """ParallelTemperingConfig(row_shared_grid=True) sets the option on the engine the run creates.  The environment's
    default for "row_shared" forces the windows (read once per engine, at its creation), so the flag decides the kernel:
    the same result from either."""
    from spin_glass_anneal_rl_amd.engine import last_kernel
    monkeypatch.setenv("SGA_ROW_SHARED", "1")
    n = 64
    J, h = quarter_problem(n, 31, amp=1, hkind="quarter")

    def run(flag):
        m = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=False))
        m.set_couplings_from_matrix(torch.from_numpy(J))
        m.set_external_fields(torch.from_numpy(h))
        cfg = sg.ParallelTemperingConfig(n_replicas=6, n_sweeps=30, temp_min=0.1, temp_max=3.0, exchange_interval=5, record_interval=5,
                                         random_seed=12, coupling_storage="f32", field_cache="off", autotune=False, row_shared_grid=flag)
        pt = sg.ParallelTempering(cfg)
        res = pt.run(m)
        return (res.best_energy, res.best_configuration.numpy().copy(), np.asarray(pt.energy_histories), pt.exchange_accepts.copy(),
                last_kernel())

    on, off = run(True), run(False)
    assert on[4].startswith("sweep_dense_rs<float, planes=1, W=1024, grid=2^-2>"), on[4]
    assert off[4].startswith("sweep_dense_kernel<"), off[4]
    for a, b in zip(on[:4], off[:4]):
        assert np.array_equal(a, b)
