"""The window forms at the limits of their number ranges (tests/range_edges.py, the window section): sequential windows
(csrc/sweep_dense_seq.hip) and row-shared windows on a binary grid (csrc/sweep_dense_rs.hip under sga_classify's
row_shared_grid).  The instance at the LAST value a set-time condition admits must run the form -- with the product's
matrix cores and the plane count its side of the limit gives --, its twin one unit beyond must not, and both walk the
oracle's chain bit for bit from the gauge state (xi, -xi, xi with the limit row flipped, random) at T = 0, L/8, L/2, 2L
and inf: energy trace, spins, tracked energies, accept counts, bests, then from-scratch energies.  No tolerances.
Sequential-order runs hand ONE recorded array of uniforms to the engine and to the oracle; random-site runs draw the
Philox stream.  tests/test_window_range_edges_host.py shows from the reference alone that these runs hold the moves at
the limit and that the set-time traits are the expected ones.

Then what the form keeps between calls: the resident int8 copy across successive problems of one engine, the product's
scratch across a change of W and of the replica count, and the model of a shared-coupling replica on a shard that
begins inside a model."""
import numpy as np
import pytest

import oracle
import range_edges as re_

pytestmark = pytest.mark.gpu

SEQ = oracle.SITE_SEQUENTIAL
W = 256


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def compare(e, out, ref):
    """Energy trace, spins, tracked energies, accept counters, per-replica bests -- then from-scratch energies."""
    R = ref["spins"].shape[0]
    assert np.array_equal(out["energy_trace"], ref["energy_trace"]), e.describe()
    assert np.array_equal(e.spins(), ref["spins"])
    assert np.array_equal(e.energies(), ref["energy"])
    assert np.array_equal(e.stats()[0], ref["n_accepted"])
    for r in range(R):
        be, bs, _ = e.best(r)
        assert be == ref["best_energy"][r] and np.array_equal(bs, ref["best_spins"][r]), r
    e.recompute_energies()
    assert np.array_equal(e.energies(), ref["scratch"])


def start(e, c):
    e.init_replicas(c["s0"].shape[0], seed=c["seed"], s0=c["s0"])
    e.set_temperatures(c["temps"])


def traits_match(e, want):
    q = e.route_query()
    for k, v in want.items():
        assert getattr(q, k) == v, (k, getattr(q, k), v)


def on_the_sequential_form(e, elem, cores, grid_k=None, rule=None):
    k, d = e.last_kernel(), e.describe()
    head = f"sweep_dense_seq<{elem}, W={W}" + (f", grid=2^-{grid_k}" if grid_k is not None else "") + (f", rule={rule}>" if rule else ">")
    assert k.startswith(head), k
    assert f"(sequential windows: product on {cores} matrix cores" in k, k
    assert f"sweep=seq-windows(W={W})" in d, d


def off_the_sequential_form(e):
    assert e.last_kernel().startswith("sweep_dense_kernel<"), e.last_kernel()
    assert "seq-windows" not in e.describe(), e.describe()


# ----------------------------------------------------------------------------- A. sequential windows, the integer class
# name -> the product's matrix cores where the form takes the instance, None where it must not
INTEGER = {"p24_in_n67": "f32", "p24_in_n579": "f32", "p24_in_n579_reversed": "f32", "p24_out_n67": None, "p24_out_n579": None,
           "i24_in": "f32", "i24_out": None, "flat127": "i8", "flat127_spike128": "f32"}


@pytest.mark.parametrize("name", sorted(INTEGER))
def test_sequential_windows_at_the_limits_of_the_integer_class(sg, name):
    """Row sums of 2^24 - 1 | 2^24 on the fp32 matrix cores (the product itself at +-L from +-xi; two K splits and three
    windows at n = 579; the limit row last in the reversed instance), and |J| = 127 | 128 at the resident int8 copy."""
    c, ref, cores = re_.window_case(name), re_.window_reference(name), INTEGER[name]
    with sg.AnnealEngine(0) as e:
        e.set_sequential_windows(W)
        e.set_dense(c["J"], c["h"], storage="f32")
        start(e, c)
        traits_match(e, re_.dense_traits(c["J"], c["h"], "f32"))
        assert (" acc=f32 " if cores else " acc=f64-exact ") in e.describe(), e.describe()
        out = e.sweep(c["sweeps"], site_mode=SEQ, replay_u=c["u"], energy_trace=True)
        if cores:
            on_the_sequential_form(e, "float", cores)
        else:
            off_the_sequential_form(e)
        compare(e, out, ref)


def test_sequential_windows_int8_rows_at_their_limit(sg):
    c, ref = re_.window_case("flat127"), re_.window_reference("flat127")
    with sg.AnnealEngine(0) as e:
        e.set_sequential_windows(W)
        e.set_dense(c["J"], c["h"], storage="i8")
        start(e, c)
        traits_match(e, re_.dense_traits(c["J"], c["h"], "i8"))
        out = e.sweep(c["sweeps"], site_mode=SEQ, replay_u=c["u"], energy_trace=True)
        on_the_sequential_form(e, "int8_t", "i8")
        compare(e, out, ref)


@pytest.mark.parametrize("how", ["glauber", "heat-bath", "metropolis-f32"])
def test_sequential_windows_rules_at_the_fp32_limit(sg, how):
    rule = {"glauber": oracle.RULE_GLAUBER, "heat-bath": oracle.RULE_HEAT_BATH}.get(how, oracle.RULE_METROPOLIS)
    arith = oracle.ARITH_F32 if how == "metropolis-f32" else oracle.ARITH_F64
    c, ref = re_.window_case("p24_in_n67"), re_.window_reference("p24_in_n67", "seq", rule, arith)
    with sg.AnnealEngine(0) as e:
        e.set_sequential_windows(W)
        e.set_dense(c["J"], c["h"], storage="f32")
        e.set_update_rule(rule)
        start(e, c)
        out = e.sweep(c["sweeps"], site_mode=SEQ, arith=arith, replay_u=c["u"], energy_trace=True)
        on_the_sequential_form(e, "float", "f32", rule=None if how == "metropolis-f32" else how)
        compare(e, out, ref)


# ----------------------------------------------------------------------------- B. sequential windows, the grid class
@pytest.mark.parametrize("name", sorted(re_.GRID))
def test_sequential_windows_at_the_limits_of_the_grid_class(sg, name):
    amp, k, M, planes, cores = re_.GRID[name]
    c, ref = re_.window_case(name), re_.window_reference(name)
    with sg.AnnealEngine(0) as e:
        e.set_option("row_shared_grid", 1)
        e.set_sequential_windows(W)
        e.set_dense(c["J"], c["h"], storage="f32")
        start(e, c)
        assert e.route_query().rs_grid == (1 + k if planes else 0)
        assert "table_m=0 " in e.describe(), e.describe()
        out = e.sweep(c["sweeps"], site_mode=SEQ, replay_u=c["u"], energy_trace=True)
        if planes:
            on_the_sequential_form(e, "float", cores, grid_k=k)
        else:
            off_the_sequential_form(e)
            assert "grid=" not in e.last_kernel(), e.last_kernel()
        compare(e, out, ref)


# ----------------------------------------------------------------------------- C. row-shared windows on the grid, random sites
@pytest.mark.parametrize("name", sorted(re_.GRID))
def test_row_shared_grid_windows_at_their_limits(sg, name):
    amp, k, M, planes, _ = re_.GRID[name]
    c, ref = re_.window_case(name, "random"), re_.window_reference(name, "random")
    with sg.AnnealEngine(0) as e:
        e.set_option("row_shared", 1)
        e.set_option("row_shared_grid", 1)
        e.set_option("row_shared_window", W)
        e.set_dense(c["J"], c["h"], storage="f32")
        start(e, c)
        assert e.route_query().rs_grid == (1 + k if planes else 0)
        if planes:
            assert f"sweep=row-shared(W={W} planes={planes} grid=2^-{k})" in e.describe(), e.describe()
        else:
            assert "row-shared" not in e.describe(), e.describe()
        out = e.sweep(c["sweeps"], energy_trace=True)
        if planes:
            assert e.last_kernel().startswith(f"sweep_dense_rs<float, planes={planes}, W={W}, grid=2^-{k}>"), e.last_kernel()
        else:
            assert e.last_kernel().startswith("sweep_dense_kernel<"), e.last_kernel()
        compare(e, out, ref)


# ----------------------------------------------------------------------------- D. one engine, successive problems
def state_of(e, traces):
    R = e.R
    bests = [e.best(r) for r in range(R)]
    return dict(energy_trace=np.concatenate(traces), spins=e.spins(), energy=e.energies().copy(), n_accepted=e.stats()[0].copy(),
                best_energy=np.asarray([b[0] for b in bests]), best_spins=np.stack([b[1] for b in bests]))


def same_state(got, want, what):
    for key in ("energy_trace", "spins", "energy", "n_accepted", "best_energy", "best_spins"):
        assert np.array_equal(got[key], want[key]), (what, key)


def oracle_calls(J, h, s0, temps, us):
    """The oracle's state after each of successive calls on one set of replicas (one recorded array per call)."""
    prob = oracle.Problem(J=J, h=h)
    s, ns = s0.copy(), re_.SWEEPS
    energy = best_e = best_s = None
    acc, traces, out = np.zeros(s0.shape[0], np.int64), [], []
    for u in us:
        ref = oracle.sweeps(prob, s, temps, ns, site_mode=SEQ, replay_u=u, energy=energy, best_energy=best_e, n_threads=8)
        if best_s is None:
            best_s = ref["best_spins"]
        else:  # (a call starts its best spins from its own start state: keep the earlier ones where no sweep improved)
            better = ref["best_energy"] < best_e
            best_s = np.where(better[:, None], ref["best_spins"], best_s)
        energy, best_e = ref["energy"], ref["best_energy"]
        acc = acc + ref["n_accepted"]
        traces.append(ref["energy_trace"])
        out.append(dict(energy_trace=np.concatenate(traces), spins=s.copy(), energy=energy.copy(), n_accepted=acc.copy(),
                        best_energy=best_e.copy(), best_spins=best_s.copy()))
    return out


def fresh_engine_calls(sg, J, h, s0, temps, us, cores):
    """The same calls on an engine of their own whose window size never changes."""
    with sg.AnnealEngine(0) as e:
        e.set_sequential_windows(W)
        e.set_dense(J, h, storage="f32")
        e.init_replicas(s0.shape[0], seed=1, s0=s0)
        e.set_temperatures(temps)
        traces = []
        for u in us:
            traces.append(e.sweep(re_.SWEEPS, site_mode=SEQ, replay_u=u, energy_trace=True)["energy_trace"])
            on_the_sequential_form(e, "float", cores)
        return state_of(e, traces)


def random_int8_problem(n):
    """Couplings over the whole int8 range, both signs of 127 present, small integer fields."""
    rng = np.random.RandomState(3)
    J = np.triu(rng.randint(-127, 128, (n, n)), 1).astype(np.float32)
    J[0, 1], J[0, 2] = -127.0, 127.0
    J = J + J.T
    return J, rng.randint(-3, 4, n).astype(np.float32)


def test_one_engine_successive_problems_on_the_sequential_form(sg):
    """The resident int8 copy belongs to ONE problem, the product's scratch to one replica set (kept while W shrinks):
    at every step the re-used engine's state equals the oracle's and a fresh engine's."""
    n, R, ns = 131, 33, re_.SWEEPS
    J1, h1, xi = re_.flat_dense(127, n)
    J3, h3, _ = re_.flat_dense(127, n, 128)
    J2, h2 = random_int8_problem(n)
    assert np.abs(J2).max() == 127 and np.count_nonzero(J2 != J1) > n * n // 2
    s0 = re_.start_spins(xi, R, 44)
    t1 = re_.temperatures(R, float(127 * (n - 1) + 1))
    t2 = re_.temperatures(R, float(np.abs(J2).sum(1).max()) / 8.0)
    us = [np.ascontiguousarray(u) for u in np.split(re_.recorded_u(R, 5 * ns, n, 44), 5, axis=1)]
    refs = {1: oracle_calls(J1, h1, s0, t1, us[:1]), 2: oracle_calls(J2, h2, s0, t2, us[1:2]),
            3: oracle_calls(J3, h3, s0, t1, us[2:5]), 5: oracle_calls(J2, h2, s0[:3], t2[:3], [np.ascontiguousarray(us[0][:3])])}
    for step, ref in refs.items():  # every run accepts and refuses
        assert 0 < ref[-1]["n_accepted"].sum() < len(ref) * ns * n * ref[-1]["spins"].shape[0], step
    assert not np.array_equal(refs[1][0]["spins"], refs[2][0]["spins"])
    with sg.AnnealEngine(0) as e:
        e.set_sequential_windows(W)

        def call(u, cores, w=W):
            tr = e.sweep(ns, site_mode=SEQ, replay_u=u, energy_trace=True)["energy_trace"]
            k = e.last_kernel()
            assert k.startswith(f"sweep_dense_seq<float, W={w}>") and f"product on {cores} matrix cores" in k, k
            return tr

        # 1. |J| = 127 as fp32: the resident int8 copy is made
        e.set_dense(J1, h1, storage="f32")
        e.init_replicas(R, seed=1, s0=s0)
        e.set_temperatures(t1)
        got = state_of(e, [call(us[0], "i8")])
        same_state(got, refs[1][0], "step 1")
        same_state(got, fresh_engine_calls(sg, J1, h1, s0, t1, us[:1], "i8"), "step 1, fresh")
        # 2. other couplings of the same size and range: their own copy, not the first problem's
        e.set_dense(J2, h2, storage="f32")
        e.init_replicas(R, seed=1, s0=s0)
        e.set_temperatures(t2)
        got = state_of(e, [call(us[1], "i8")])
        same_state(got, refs[2][0], "step 2")
        same_state(got, fresh_engine_calls(sg, J2, h2, s0, t2, us[1:2], "i8"), "step 2, fresh")
        # 3. one coupling of 128: the fp32 matrix cores, no copy
        e.set_dense(J3, h3, storage="f32")
        e.init_replicas(R, seed=1, s0=s0)
        e.set_temperatures(t1)
        traces = [call(us[2], "f32")]
        same_state(state_of(e, traces), refs[3][0], "step 3")
        # 4. the same replicas: W grows (the scratch is made anew), then shrinks (kept, at the new stride)
        e.set_sequential_windows(1024)
        traces.append(call(us[3], "f32", 1024))
        same_state(state_of(e, traces), refs[3][1], "step 4, W = 1024")
        e.set_sequential_windows(W)
        traces.append(call(us[4], "f32"))
        got = state_of(e, traces)
        same_state(got, refs[3][2], "step 4, W = 256")
        same_state(got, fresh_engine_calls(sg, J3, h3, s0, t1, us[2:5], "f32"), "steps 3 and 4, fresh")
        # 5. 33 replicas -> 3, back on the second problem (its int8 copy is made again)
        e.set_dense(J2, h2, storage="f32")
        e.init_replicas(3, seed=1, s0=s0[:3])
        e.set_temperatures(t2[:3])
        u5 = np.ascontiguousarray(us[0][:3])
        got = state_of(e, [call(u5, "i8")])
        same_state(got, refs[5][0], "step 5")
        same_state(got, fresh_engine_calls(sg, J2, h2, s0[:3], t2[:3], [u5], "i8"), "step 5, fresh")


def test_one_engine_33_replicas_then_3_on_one_problem(sg):
    """init_replicas alone (no new problem): the scratch of 33 replicas goes with them, the int8 copy stays."""
    n, ns = 131, re_.SWEEPS
    J, h = random_int8_problem(n)
    s0 = re_.start_spins(re_.gauge(n).astype(np.int8), 33, 44)
    temps = re_.temperatures(33, float(np.abs(J).sum(1).max()) / 8.0)
    u = re_.recorded_u(33, ns, n, 44)
    u3 = np.ascontiguousarray(u[:3])
    want33, want3 = oracle_calls(J, h, s0, temps, [u])[0], oracle_calls(J, h, s0[:3], temps[:3], [u3])[0]
    assert all(0 < a < ns * n for a in want3["n_accepted"])
    with sg.AnnealEngine(0) as e:
        e.set_sequential_windows(W)
        e.set_dense(J, h, storage="f32")
        for R, uu, want in ((33, u, want33), (3, u3, want3)):
            e.init_replicas(R, seed=1, s0=s0[:R])
            e.set_temperatures(temps[:R])
            tr = e.sweep(ns, site_mode=SEQ, replay_u=uu, energy_trace=True)["energy_trace"]
            on_the_sequential_form(e, "float", "i8")
            same_state(state_of(e, [tr]), want, R)


# ----------------------------------------------------------------------------- E. shared couplings, a shard cut inside a model
def test_shared_couplings_on_a_shard_that_begins_inside_a_model(sg):
    """3 models x 4 replicas over one J, the shard holds global replicas 3 ... 7: the last replica of model 0 and all of
    model 1, whose field makes row 0's bound 2^24 - 1.  The chain finds a replica's h as (replica0 + r) / 4."""
    n, M, k, r0, Rl, ns, seed = 67, 3, 4, 3, 5, re_.SWEEPS, 44
    L = (1 << 24) - 1
    J, _, xi = re_.product_saturating_dense(L - 3, n)
    rng = np.random.RandomState(9)
    hs = rng.randint(-3, 4, (M, n)).astype(np.float32)
    hs[1, 0] = 3.0 * xi[0]
    hs[0, 0], hs[2, 0] = -2.0 * xi[0], 0.0
    bounds = np.abs(J).astype(np.float64).sum(1)[None, :] + np.abs(hs)
    assert bounds.max() == bounds[1, 0] == L and not np.array_equal(hs[0], hs[1])
    s0 = np.concatenate([re_.start_spins(xi, k, seed + m) for m in range(M)])
    temps = np.tile(re_.temperatures(k, float(L)), M)
    u = re_.recorded_u(M * k, ns, n, seed)
    sl = slice(r0, r0 + Rl)
    with sg.AnnealEngine(0) as e:
        e.set_sequential_windows(W)
        e.set_dense_shared(J, hs, storage="f32")
        e.init_replicas(Rl, seed=seed, s0=np.ascontiguousarray(s0[sl]), R_global=M * k, replica0=r0)
        e.set_temperatures(temps[sl])
        assert f"shared-J models={M}" in e.describe(), e.describe()
        out = e.sweep(ns, site_mode=SEQ, replay_u=np.ascontiguousarray(u[sl]), energy_trace=True)
        on_the_sequential_form(e, "float", "f32")
        got = state_of(e, [out["energy_trace"]])
        e.recompute_energies()
        scratch = e.energies().copy()
    for m in range(M):
        prob = oracle.Problem(J=J, h=hs[m])
        s = s0[m * k:(m + 1) * k].copy()
        ref = oracle.sweeps(prob, s, temps[m * k:(m + 1) * k], ns, site_mode=SEQ, replay_u=np.ascontiguousarray(u[m * k:(m + 1) * k]),
                            seed=seed, replica0=m * k, n_threads=4)
        ref["spins"], ref["scratch"] = s, oracle.energy(prob, s)
        for g in range(max(m * k, r0), min((m + 1) * k, r0 + Rl)):  # global replica g: local g - r0, g - m k of its model
            a, b = g - r0, g - m * k
            if temps[g] > 0.0:
                assert 0 < ref["n_accepted"][b] < ns * n, g
            assert np.array_equal(got["energy_trace"][:, a], ref["energy_trace"][:, b]), g
            assert np.array_equal(got["spins"][a], ref["spins"][b]), g
            for key in ("energy", "n_accepted", "best_energy", "best_spins"):
                assert np.array_equal(got[key][a], ref[key][b]), (g, key)
            assert scratch[a] == ref["scratch"][b], g
