"""Replica groups of the row-shared sweep (sga_set_replica_groups; csrc/sweep_dense_rs.hip, launch_sweep_dense_rs): over
the tile plan, contiguous ranges of replicas run the whole sweep as engines of their own, a stream each, forked from the
engine's stream and joined into it.  None of it may show in a result: spins, energies, acceptance counters, temperatures
and best states under 2 and 4 groups equal -- to the bit -- the same build at one group and the CPU oracle.  Every run asks
for "row_shared" = 1 and "row_shared_fields" = 1 with tiles small enough for a dozen of them, so that the tile plan runs
at small n, and asserts from last_kernel() / describe() that the groups it expects ran (the expectation is the host rule's,
tests/test_replica_groups_host.py).  No run asks for an energy trace, which takes one group, but the test of just that."""
import functools
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batch_fx_cases import oracle_batch  # noqa: E402
from oracle_engine import OracleEngine  # noqa: E402
from test_replica_groups_host import expected_ranges  # noqa: E402
from test_sequential_windows_gpu import philox_u  # noqa: E402
from test_row_shared_tiles_gpu import INF, assert_kernel, assert_same, couplings, fields, ladder, select, state, temps_for  # noqa: E402

pytestmark = pytest.mark.gpu

SCRIPT = (2, 1, 2)  # sweeps, an exchange round between the blocks
SHAPES = {300: (256, 24), 1100: (1024, 96)}  # n: (W, S) -- one full window and a cut one of 13 tiles; one cut window of 12


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def full_state(e, R):
    return dict(state(e, R), temps=np.asarray(e.temperatures()))


def run(e, R, script):
    for i, ns in enumerate(script):
        e.sweep(ns)
        if i + 1 < len(script):
            e.exchange()
    return full_state(e, R)


def assert_groups(e, R, G, S, ones=None):
    """The groups the host rule gives for (R, G asked for) ran, and the strings of one group are what they were."""
    want = len(expected_ranges(R, G))
    assert_kernel(e, "tiles", S, ones)
    kernel, desc = e.last_kernel(), e.describe()
    if want > 1:
        assert kernel.endswith(f" groups={want}") and desc.endswith(f" groups={want}"), (kernel, desc)
    elif G > 1:  # more were asked for than 32 replicas or fewer give: one group, and sga_describe says why
        assert "groups=" not in kernel and desc.endswith(" groups=no(32 replicas or fewer)"), (kernel, desc)
    else:
        assert "groups=" not in kernel and "groups=" not in desc, (kernel, desc)


def engine_run(sg, J, h, R, W, S, storage, temps, seed, script, G, ones=None, spl=0, rule=None):
    with sg.AnnealEngine(0) as e:
        select(e, "tiles", W, S)
        e.set_replica_groups(G)
        assert e.replica_groups() == G
        if spl:
            e.set_tuning(sweeps_per_launch=spl)
        if rule is not None:
            e.set_update_rule(rule)
        e.set_dense(J, h, storage=storage)
        e.init_replicas(R, seed=seed)
        e.set_ladder(temps)
        out = run(e, R, script)
        assert_groups(e, R, G, S, ones)
    return out


def problem(n, kind, R):
    jseed = 29 + n + R
    return couplings(n, kind, jseed), fields(n, kind, n), temps_for(n, R, kind), 2000 + n + R


@functools.lru_cache(maxsize=None)
def oracle_run(n, kind, R, script):
    J, h, temps, seed = problem(n, kind, R)
    one_thread = oracle.sweeps
    oracle.sweeps = functools.partial(one_thread, n_threads=16)
    try:
        o = OracleEngine(J=np.array(J), h=np.array(h))
        o.init_replicas(R, seed=seed)
        o.set_ladder(temps)
        return run(o, R, script)
    finally:
        oracle.sweeps = one_thread


@functools.lru_cache(maxsize=None)
def one_group_run(n, kind, R, storage, script, spl=0):
    import spin_glass_anneal_rl_amd as sg
    J, h, temps, seed = problem(n, kind, R)
    W, S = SHAPES[n]
    return engine_run(sg, J, h, R, W, S, storage, temps, seed, script, 1, spl=spl)


def check_case(sg, n, kind, R, G, storage="f32", ones=None, script=SCRIPT, spl=0):
    J, h, temps, seed = problem(n, kind, R)
    W, S = SHAPES[n]
    new = engine_run(sg, J, h, R, W, S, storage, temps, seed, script, G, ones, spl)
    assert_same(new, one_group_run(n, kind, R, storage, script, spl), "one group")
    assert_same(new, oracle_run(n, kind, R, script), "oracle")
    return new


# ----------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("R", [1, 33, 70, 130])
@pytest.mark.parametrize("n", [300, 1100])
def test_shapes(sg, n, R, G):
    """One replica (one group whatever is asked), a second group of one replica, three ranges where four are asked for, a
    last range of 34; n = 300: a full window and one of 44 updates, n = 1100: a window of 76 behind a full one."""
    check_case(sg, n, "pm1", R, G, ones=True)


# ----------------------------------------------------------------------------- rows
@pytest.mark.parametrize("kind,storage", [("pm1-hole", "f32"), ("a7", "f32"), ("pm1", "i8"), ("a7", "i8")])
def test_rows(sg, kind, storage):
    """One general magnitude plane (a pair set to 0), three planes, int8 storage; sign-only fp32 rows: test_shapes."""
    check_case(sg, 300, kind, 70, 4, storage=storage, ones=(kind == "pm1"))


def test_glauber(sg):
    n, R, ns = 300, 70, 3
    J, h, temps, seed = problem(n, "pm1", R)
    W, S = SHAPES[n]
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(oracle.Problem(J=np.array(J), h=np.array(h)), s, temps, ns, rule=oracle.RULE_GLAUBER, seed=seed, n_threads=16)
    got = {G: engine_run(sg, J, h, R, W, S, "f32", temps, seed, (ns,), G, ones=True, rule=sg._native.RULE_GLAUBER) for G in (1, 4)}
    assert_same(got[4], got[1], "one group")
    assert np.array_equal(got[4]["spins"], s) and np.array_equal(got[4]["energy"], ref["energy"])
    assert np.array_equal(got[4]["accepted"], ref["n_accepted"])
    assert np.array_equal(got[4]["best_energy"], ref["best_energy"]) and np.array_equal(got[4]["best_spins"], ref["best_spins"])


# ----------------------------------------------------------------------------- sweep boundaries
@pytest.mark.parametrize("G", [2, 4])
def test_several_sweeps_in_one_launch(sg, G):
    """sweeps_per_launch = 3: the groups do not join between the sweeps of a launch, a group whose replicas are cold runs
    ahead of the others across the boundary (its own plan, bits and best tracking)."""
    check_case(sg, 300, "pm1", 130, G, ones=True, script=(3, 3, 2), spl=3)


def test_zero_and_infinite_temperature_in_different_groups(sg):
    """A schedule per replica (its pointer advances with the group): T = inf and T = 0 replicas in each of the three ranges."""
    n, R, ns, seed = 300, 70, 4, 5
    W, S = SHAPES[n]
    J, h = couplings(n, "pm1", 8), fields(n, "pm1", n)
    sched = np.tile(np.resize(np.asarray([INF, 0.0, 10.0, 1.25, 0.0, INF, 3.0]), R), (ns, 1))
    assert sched[0, 0] == sched[0, 35] == sched[0, 68] == INF and sched[0, 1] == sched[0, 36] == sched[0, 64] == 0.0
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(oracle.Problem(J=np.array(J), h=np.array(h)), s, sched, ns, seed=seed, n_threads=16)
    assert ref["n_accepted"][0] == ref["n_accepted"][35] == ns * n
    got = {}
    for G in (1, 4):
        with sg.AnnealEngine(0) as e:
            select(e, "tiles", W, S)
            e.set_replica_groups(G)
            e.set_dense(J, h, storage="f32")
            e.init_replicas(R, seed=seed)
            e.sweep(ns, sched=sched)
            assert_groups(e, R, G, S, ones=True)
            got[G] = full_state(e, R)
    assert_same(got[4], got[1], "one group")
    assert np.array_equal(got[4]["spins"], s) and np.array_equal(got[4]["energy"], ref["energy"])
    assert np.array_equal(got[4]["accepted"], ref["n_accepted"])
    assert np.array_equal(got[4]["best_energy"], ref["best_energy"]) and np.array_equal(got[4]["best_spins"], ref["best_spins"])


# ----------------------------------------------------------------------------- shards of a shared-coupling batch
@pytest.mark.parametrize("k,M,r0,where", [(32, 4, 32, "at"), (20, 5, 20, "inside")])
def test_shared_coupling_shard(sg, k, M, r0, where):
    """sga_set_dense_shared, M field vectors x k replicas over one +-1 matrix, the replicas from r0 on as a shard of their
    own: Philox coordinates and the model of a replica are global (replica0 + r), the groups local.  k = 32: the models
    change at the group boundaries (local 32, 64); k = 20: inside the groups (local 20, 40 in [0, 32) and [32, 80))."""
    n, seed, plan = 300, 0x711E7, (2, 1)
    W, S = SHAPES[n]
    R = M * k
    Rl = R - r0
    ranges = expected_ranges(Rl, 4)
    bounds = {b for _, b in ranges[:-1]}
    models = {m * k - r0 for m in range(1, M) if m * k > r0}
    assert (models == bounds) if where == "at" else (len(ranges) > 1 and not models & bounds and models)
    J = np.array(couplings(n, "pm1", 8))
    hs = np.stack([np.random.RandomState(70 + m).randint(-1, 2, n).astype(np.float32) for m in range(M)])
    temps = np.tile(ladder(k, 26.0, 2.6), M)
    ref = oracle_batch(np.ascontiguousarray(np.broadcast_to(J, (M,) + J.shape)), hs, k, seed, temps, plan, exchange=False)
    got = {}
    for G in (1, 4):
        with sg.AnnealEngine(0) as e:
            select(e, "tiles", W, S)
            e.set_replica_groups(G)
            e.set_dense_shared(J, hs, storage="f32")
            e.init_replicas(Rl, seed=seed, R_global=R, replica0=r0)
            e.set_temperatures(temps[r0:])
            for ns in plan:
                e.sweep(ns)
            assert_groups(e, Rl, G, S, ones=True)
            got[G] = full_state(e, Rl)
    assert_same(got[4], got[1], "one group")
    assert np.array_equal(got[4]["energy"], np.concatenate(ref["traces"])[-1, r0:])
    assert np.array_equal(got[4]["spins"], ref["spins"][r0:]) and np.array_equal(got[4]["accepted"], ref["acc"][r0:])
    assert np.array_equal(got[4]["best_energy"], ref["best_e"][r0:]) and np.array_equal(got[4]["best_spins"], ref["best_s"][r0:])


# ----------------------------------------------------------------------------- the join
def test_energy_trace_takes_one_group(sg):
    """The trace is strided by all replicas: a call that asks for it runs one group and is the oracle's; the next call
    without one runs its groups again."""
    n, R = 300, 70
    J, h, temps, seed = problem(n, "pm1", R)
    W, S = SHAPES[n]
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(oracle.Problem(J=np.array(J), h=np.array(h)), s, temps, 3, seed=seed, n_threads=16)
    with sg.AnnealEngine(0) as e:
        select(e, "tiles", W, S)
        e.set_replica_groups(4)
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_temperatures(temps)
        a = e.sweep(2, energy_trace=True)["energy_trace"]
        assert "groups=" not in e.last_kernel(), e.last_kernel()
        e.sweep(1)
        assert e.last_kernel().endswith(" groups=3"), e.last_kernel()
        assert np.array_equal(a, ref["energy_trace"][:2]) and np.array_equal(e.energies(), ref["energy"])
        assert np.array_equal(e.spins(), s) and np.array_equal(e.stats()[0], ref["n_accepted"])


def test_what_follows_the_sweep_sees_every_group(sg):
    """Work queued right behind the sweep -- the energies read on another stream once the engine's stream is done, an
    exchange round, best tracking -- finds every group's replicas finished: the engine runs on a stream of the caller's,
    and a second stream that only waits for an event recorded behind the sweep reads the state."""
    import torch
    n, R = 1100, 130
    J, h, temps, seed = problem(n, "pm1", R)
    W, S = SHAPES[n]
    want = one_group_run(n, "pm1", R, "f32", (2,))
    main, side = torch.cuda.Stream(), torch.cuda.Stream()
    with sg.AnnealEngine(0) as e:
        e.use_stream(main.cuda_stream)
        select(e, "tiles", W, S)
        e.set_replica_groups(4)
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_ladder(temps)
        out = torch.zeros(R, dtype=torch.float64, device="cuda")
        main.synchronize()
        with torch.cuda.stream(main):
            e.sweep(2)
            e.energies_into(out, stream_ordered=True)  # on the engine's stream, no host synchronisation
            done = torch.cuda.Event()
            done.record(main)
        side.wait_event(done)
        with torch.cuda.stream(side):
            seen = out.clone()
        side.synchronize()
        assert_groups(e, R, 4, S, ones=True)
        assert np.array_equal(seen.cpu().numpy(), want["energy"])
        assert_same(full_state(e, R), want, "one group")
        # an exchange round right behind a grouped sweep decides on the joined energies
        e.sweep(1)
        swaps = e.exchange()
    with sg.AnnealEngine(0) as e1:
        select(e1, "tiles", W, S)
        e1.set_replica_groups(1)
        e1.set_dense(J, h, storage="f32")
        e1.init_replicas(R, seed=seed)
        e1.set_ladder(temps)
        e1.sweep(2)
        e1.sweep(1)
        assert e1.exchange() == swaps


def test_autotune_in_mid_run_leaves_no_trace(sg):
    """sga_autotune's window trials run under the groups the caller forced, on the live replicas; the chain goes on as if
    they had not."""
    n, R = 1100, 70
    J, h, temps, seed = problem(n, "pm1", R)
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(oracle.Problem(J=np.array(J), h=np.array(h)), s, temps, 3, seed=seed, n_threads=16)
    with sg.AnnealEngine(0) as e:
        e.set_option("row_shared_fields", 1)
        e.set_option("row_shared_tile_sites", 96)
        e.set_replica_groups(4)
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_temperatures(temps)
        e.sweep(1)
        before = (e.spins(), e.energies(), e.best()[0], e.stats()[0], e.counters(), e.temperatures())
        e.autotune()
        after = (e.spins(), e.energies(), e.best()[0], e.stats()[0], e.counters(), e.temperatures())
        for x, y in zip(before, after):
            assert np.array_equal(np.asarray(x), np.asarray(y))
        assert {k for k in e.autotune_table(forms=True) if k.startswith("row-shared:")} == {"row-shared:W256", "row-shared:W512", "row-shared:W1024"}
        e.sweep(2)
        if "sweep=row-shared(W=" in e.describe():  # (which form wins is a measurement)
            assert e.last_kernel().endswith(" groups=3") and e.describe().endswith(" groups=3"), (e.last_kernel(), e.describe())
        assert np.array_equal(e.energies(), ref["energy"]) and np.array_equal(e.spins(), s)
        assert np.array_equal(e.stats()[0], ref["n_accepted"])
        for r in range(R):
            be, bs, _ = e.best(r)
            assert be == ref["best_energy"][r] and np.array_equal(bs, ref["best_spins"][r])


def test_two_runs_leave_identical_state(sg):
    n, R = 1100, 130
    J, h, temps, seed = problem(n, "pm1", R)
    W, S = SHAPES[n]
    a = engine_run(sg, J, h, R, W, S, "f32", temps, seed, SCRIPT, 4, ones=True)
    b = engine_run(sg, J, h, R, W, S, "f32", temps, seed, SCRIPT, 4, ones=True)
    assert_same(a, b, "second run")


# ----------------------------------------------------------------------------- forms without groups, the setter
def test_forms_without_groups_ignore_the_setter_and_say_so(sg):
    n, R = 300, 70
    J, h, temps, seed = problem(n, "pm1", R)
    want = one_group_run(n, "pm1", R, "f32", (2,))
    with sg.AnnealEngine(0) as e:  # the per-site fields kernel
        select(e, "site", 256)
        e.set_replica_groups(4)
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_ladder(temps)
        e.sweep(2)
        assert_kernel(e, "site")
        assert "groups=" not in e.last_kernel() and " groups=no(the per-site fields kernel" in e.describe(), (e.last_kernel(), e.describe())
        assert_same(full_state(e, R), want, "per-site kernel")
        e.set_replica_groups(0)
        assert "groups=" not in e.describe()
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(oracle.Problem(J=np.array(J), h=np.array(h)), s, temps, 2, site_mode=oracle.SITE_SEQUENTIAL,
                        replay_u=philox_u(seed, R, 2, n), seed=seed, n_threads=16)  # (the oracle's own stream, recorded)
    with sg.AnnealEngine(0) as e:  # the sequential windows
        e.set_option("row_shared", 0)
        e.set_sequential_windows(256)
        e.set_replica_groups(2)
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_temperatures(temps)
        e.sweep(2, site_mode=sg._native.SITE_SEQUENTIAL)
        assert e.last_kernel().startswith("sweep_dense_seq<") and "groups=" not in e.last_kernel(), e.last_kernel()
        assert " sweep=seq-windows(W=256)" in e.describe() and e.describe().endswith(" groups=no(not the row-shared windows)"), e.describe()
        assert np.array_equal(e.spins(), s) and np.array_equal(e.energies(), ref["energy"])
        assert np.array_equal(e.stats()[0], ref["n_accepted"])


def test_the_setter_refuses_other_counts(sg):
    with sg.AnnealEngine(0) as e:
        assert e.replica_groups() == 0
        for g in (-1, 3, 5, 8):
            with pytest.raises(sg.AnnealingError, match="replica groups"):
                e.set_replica_groups(g)
        for g in (1, 2, 4, 0):
            e.set_replica_groups(g)
            assert e.replica_groups() == g
