"""Row-shared windows (csrc/sweep_dense_rs.hip, option "row_shared"): the dense sweep of integer problems that reads
each proposed coupling row once per window of W updates per replica and walks the chain per replica with exact
corrections for the window's earlier accepts.  The same chain bit for bit as the oracle's strictly sequential one and
as the kernel it replaces -- repeated sites inside a window, windows cut by the end of a sweep, several sweeps and
exchanges, T = 0 and T = inf -- and the problems the form does not serve fall back to that kernel."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

INF = float("inf")


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def int_couplings(n, seed, amp, density=1.0):
    rng = np.random.RandomState(seed)
    J = np.triu(rng.randint(-amp, amp + 1, (n, n)) * (rng.rand(n, n) < density), 1).astype(np.float32)
    if amp == 1 and density == 1.0:
        J = np.triu(rng.randint(0, 2, (n, n)) * 2 - 1, 1).astype(np.float32)
    return J + J.T


def ladder(R, tmax, tmin):
    return np.asarray([tmax * (tmin / tmax) ** (i / max(R - 1, 1)) for i in range(R)])


def forced(e, W=0, on=True):
    e.set_option("row_shared", 1 if on else 0)
    e.set_option("row_shared_window", W)


def check_against(e, ref, s, out, R):
    assert np.array_equal(out["energy_trace"], ref["energy_trace"])
    assert np.array_equal(e.spins(), s)
    assert np.array_equal(e.stats()[0], ref["n_accepted"])
    for r in range(R):
        be, bs, _ = e.best(r)
        assert be == ref["best_energy"][r] and np.array_equal(bs, ref["best_spins"][r])


@pytest.mark.parametrize("n,R,storage,amp,W", [
    (3, 4, "f32", 1, 256), (7, 5, "i8", 1, 512), (64, 8, "f32", 1, 1024),   # many repeated sites inside a window
    (300, 1, "f32", 5, 256),                                                 # one replica, |J| up to 5
    (1000, 6, "i8", 5, 256), (2500, 3, "f32", 3, 512), (1500, 2, "f32", 100, 1024),  # n not a multiple of W / 64 / a chunk
    (700, 3, "t2", 1, 256), (5000, 4, "t2", 1, 1024),                        # ternary couplings (bit-plane storage)
    (10000, 64, "f32", 1, 1024),                                             # the headline's size at 64 replicas
])
def test_row_shared_equals_the_oracle(sg, n, R, storage, amp, W):
    from spin_glass_anneal_rl_amd.engine import last_kernel
    rng = np.random.RandomState(n + amp)
    J = int_couplings(n, 5 + n, amp, density=0.6 if storage == "t2" else 1.0)
    h = rng.randint(-3, 4, n).astype(np.float32)
    prob = oracle.Problem(J=J, h=h)
    ns, seed = 3 if n >= 5000 else 5, 777 + n
    temps = ladder(R, 2.0 * amp * np.sqrt(n), 0.3)
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(prob, s, temps, ns, seed=seed, n_threads=8)
    with sg.AnnealEngine(0) as e:
        forced(e, W)
        e.set_dense(J, h, storage=storage)
        e.init_replicas(R, seed=seed)
        assert f"sweep=row-shared(W={W} " in e.describe(), e.describe()
        assert "look_ahead=" in e.describe()
        e.set_temperatures(temps)
        out = e.sweep(ns, energy_trace=True)
        assert last_kernel().startswith("sweep_dense_rs<"), last_kernel()
        check_against(e, ref, s, out, R)


def test_several_sweeps_and_exchanges_equal_the_kernel_it_replaces(sg):
    n, R, seed = 1200, 16, 99
    J = int_couplings(n, 3, 2)
    h = np.random.RandomState(4).randint(-2, 3, n).astype(np.float32)
    temps = ladder(R, 60.0, 0.5)
    runs = {}
    for on in (True, False):
        with sg.AnnealEngine(0) as e:
            forced(e, 256, on)
            e.set_dense(J, h, storage="f32")
            e.init_replicas(R, seed=seed)
            e.set_ladder(temps)
            trace, swaps = [], []
            for k in range(4):
                trace.append(e.sweep(3, energy_trace=True)["energy_trace"])
                swaps.append(e.exchange())
            assert ("sweep=row-shared" in e.describe()) == on
            runs[on] = (np.vstack(trace), swaps, e.spins(), e.energies(), e.best()[0], e.stats()[0])
    for a, b in zip(runs[True], runs[False]):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_zero_and_infinite_temperature_equal_the_oracle(sg):
    n, R, ns, seed = 900, 6, 6, 5
    J = int_couplings(n, 8, 3)
    h = np.random.RandomState(9).randint(-2, 3, n).astype(np.float32)
    sched = np.tile(np.asarray([INF, 0.0, 40.0, 5.0, 0.0, INF]), (ns, 1))
    sched[3:, 2] = 0.0
    prob = oracle.Problem(J=J, h=h)
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(prob, s, sched, ns, seed=seed, n_threads=8)
    with sg.AnnealEngine(0) as e:
        forced(e, 512)
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        out = e.sweep(ns, sched=sched, energy_trace=True)
        check_against(e, ref, s, out, R)
    acc = ref["n_accepted"]
    assert acc[0] == acc[5] == ns * n  # T = inf accepts every proposal


@pytest.mark.parametrize("case", ["gauss", "asymmetric", "traces", "batch", "large_J"])
def test_problems_the_form_does_not_serve_fall_back_with_the_same_chain(sg, case):
    from spin_glass_anneal_rl_amd.engine import last_kernel
    n, R, ns, seed = 500, 4, 3, 21
    rng = np.random.RandomState(2)
    J = int_couplings(n, 6, 1)
    if case == "gauss":
        J = np.triu(rng.randn(n, n), 1).astype(np.float32)
        J = J + J.T
    elif case == "asymmetric":
        J = J.copy()
        J[0, 1] = -J[1, 0]
    elif case == "large_J":
        J = int_couplings(n, 6, 300)
    h = rng.randint(-1, 2, n).astype(np.float32)
    temps = ladder(R, 30.0, 0.5)
    s = oracle.init_spins(n, R, seed)
    with sg.AnnealEngine(0) as e:
        forced(e, 256)
        if case == "batch":
            e.set_dense_batch(np.stack([J, J]), np.stack([h, h]), storage="f32")
            e.init_replicas(2 * R, seed=seed)
            e.set_temperatures(np.concatenate([temps, temps]))
            e.sweep(ns)
            assert last_kernel().startswith("sweep_dense_kernel<"), last_kernel()
            assert "sweep=row-shared" not in e.describe()
            return
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_temperatures(temps)
        out = e.sweep(ns, energy_trace=True, trace=case == "traces")
        assert last_kernel().startswith("sweep_dense_kernel<"), last_kernel()
        if case != "traces":
            assert "sweep=row-shared" not in e.describe()
        ref = oracle.sweeps(oracle.Problem(J=J, h=h), s, temps, ns, seed=seed, n_threads=8,
                            recompute_energy=case == "asymmetric")  # (asymmetric J: energies recomputed per sweep)
        assert np.array_equal(out["energy_trace"], ref["energy_trace"])
        assert np.array_equal(e.spins(), s)


@pytest.mark.parametrize("n,R,must_pick", [(10000, 256, True), (2000, 1024, False)])
def test_autotune_keeps_the_chain_and_the_state_when_it_picks_the_form(sg, n, R, must_pick):
    """sga_autotune times the row-shared windows beside the geometries (option "row_shared" = 2) and keeps the form
    exactly where it beats the fastest geometry by more than 1 %: on C2a's 400 MB of couplings (beyond the Infinity
    Cache) it does by far; on a 16 MB matrix the row-per-proposal kernel is served from the caches and may stay.  Either
    way the run continues exactly as the oracle's uninterrupted one."""
    from spin_glass_anneal_rl_amd.engine import last_kernel
    seed = 4242
    J = int_couplings(n, 11, 1)
    h = np.random.RandomState(1).randint(-1, 2, n).astype(np.float32)
    temps = ladder(R, 10.0, 0.1)  # (bench.py's ladder)
    prob = oracle.Problem(J=J, h=h)
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(prob, s, temps, 5, seed=seed, n_threads=16)
    with sg.AnnealEngine(0) as e:
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_ladder(temps)
        a = e.sweep(2, energy_trace=True)
        assert last_kernel().startswith("sweep_dense_kernel<")  # (option "row_shared" = 2: not before the autotuner)
        ms = e.autotune()
        table = e.autotune_table(forms=True)
        forms = {k: v for k, v in table.items() if k.startswith("row-shared:")}
        geometries = e.autotune_table()
        assert set(forms) == {"row-shared:W256", "row-shared:W512", "row-shared:W1024"}
        assert not set(forms) & set(geometries) and ms == pytest.approx(min(geometries.values()), rel=1e-3)
        # (the table is printed to 4 decimals: a candidate sitting exactly on the 1 % line may fall either way)
        best_form, best_geometry = min(forms.values()), min(geometries.values())
        picked = "sweep=row-shared(W=" in e.describe()
        if must_pick:
            assert picked and best_form < 0.5 * best_geometry, table
        elif best_form < 0.989 * best_geometry:
            assert picked, table
        elif best_form > 0.991 * best_geometry:
            assert not picked, table
        b = e.sweep(3, energy_trace=True)
        if picked:
            W = int(min(forms, key=forms.get)[len("row-shared:W"):])
            assert f"sweep=row-shared(W={W} " in e.describe(), (e.describe(), table)
            assert last_kernel().startswith(f"sweep_dense_rs<float, planes=1, W={W}>"), last_kernel()
        else:
            assert last_kernel().startswith("sweep_dense_kernel<"), last_kernel()
        assert np.array_equal(np.concatenate([a["energy_trace"], b["energy_trace"]]), ref["energy_trace"])
        assert np.array_equal(e.spins(), s)
        assert np.array_equal(e.stats()[0], ref["n_accepted"])
        assert e.counters()[0] == 5
        for r in range(R):
            be, bs, _ = e.best(r)
            assert be == ref["best_energy"][r] and np.array_equal(bs, ref["best_spins"][r])
