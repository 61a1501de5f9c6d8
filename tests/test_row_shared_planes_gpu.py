"""Row-shared windows with the bit-planes of J resident in HBM and the window plan histogrammed in LDS
(csrc/sweep_dense_rs.hip): the fields come from planes made once per problem, the chain's correction is gathered from
them where J is ternary, and the plan is a counting sort per (window, replica group, tile of 16384 sites) without an
atomic that reaches memory.  None of it may show in a result: spins, energies, accept counters, best energies and best
spins are equal -- not close -- to the CPU oracle's (tests/oracle_engine.py) and to the same engine on the
row-per-proposal kernel, at the edges of the bit layout, with ragged replica groups, on both field sources, on both
sides of the plan's tile bound, across a second set_dense (stale planes), another replica count and an autotune."""
import functools
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_engine import OracleEngine  # noqa: E402

pytestmark = pytest.mark.gpu

PLAN_TILE = 16384  # RS_PLAN_TILE of sweep_dense_rs.hip: sites per tile of the plan's LDS histogram


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def couplings(n, kind, seed):
    """Symmetric, zero diagonal, integer valued (int8 arithmetic: n up to 16385 stays cheap).  kind: "pm1" (+-1, dense),
    "tern" (ternary, ~70 % zeros), "a7" (|J| <= 7), "a100" (|J| <= 100)."""
    rng = np.random.RandomState(seed)
    if kind == "pm1":
        A = (rng.randint(0, 2, (n, n), dtype=np.int8) * 2 - 1).astype(np.int8)
    elif kind == "tern":
        A = rng.randint(-1, 2, (n, n), dtype=np.int8) * (rng.randint(0, 100, (n, n), dtype=np.int8) < 45)
    else:
        amp = 7 if kind == "a7" else 100
        A = rng.randint(-amp, amp + 1, (n, n), dtype=np.int8)
    A = np.triu(A.astype(np.int8), 1)
    return (A + A.T).astype(np.float32)


def fields(n, kind, seed):
    amp = 3 if kind == "a100" else 1
    return np.random.RandomState(seed + 1).randint(-amp, amp + 1, n).astype(np.float32)


def ladder(R, tmax, tmin):
    return np.asarray([tmax * (tmin / tmax) ** (i / max(R - 1, 1)) for i in range(R)])


def temps_for(n, R, kind):
    amp = {"pm1": 1, "tern": 1, "a7": 7, "a100": 100}[kind]
    return ladder(R, 2.0 * amp * np.sqrt(n), 0.3)


def forced(e, W, on=True):
    e.set_option("row_shared", 1 if on else 0)
    e.set_option("row_shared_window", W)


def state(e, R):
    """Everything a run leaves behind, as arrays."""
    best = [e.best(r) for r in range(R)]
    return {"spins": np.asarray(e.spins()), "energy": np.asarray(e.energies()), "accepted": np.asarray(e.stats()[0]),
            "best_energy": np.asarray([b[0] for b in best]), "best_spins": np.stack([np.asarray(b[1]) for b in best])}


def assert_same(a, b, what=""):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


def run(e, R, script):
    """script: a list of sweep counts; an exchange round follows each block but the last."""
    trace = []
    for i, ns in enumerate(script):
        trace.append(e.sweep(ns, energy_trace=True)["energy_trace"])
        if i + 1 < len(script):
            e.exchange()
    out = state(e, R)
    out["trace"] = np.vstack(trace)
    return out


def engine_run(sg, J, h, R, W, storage, on, temps, seed, script, source=None):
    from spin_glass_anneal_rl_amd.engine import last_kernel
    with sg.AnnealEngine(0) as e:
        forced(e, W, on)
        e.set_dense(J, h, storage=storage)
        e.init_replicas(R, seed=seed)
        e.set_ladder(temps)
        out = run(e, R, script)
        if on:
            assert f"sweep=row-shared(W={W} planes=" in e.describe(), e.describe()
            assert last_kernel().startswith("sweep_dense_rs<"), last_kernel()
            if source:
                assert f"fields from {source}" in last_kernel(), last_kernel()
        else:
            assert last_kernel().startswith("sweep_dense_kernel<"), last_kernel()
    return out


def oracle_run(J, h, R, temps, seed, script):
    """The script on the test double; its sweeps on 16 threads (replicas are independent: same chain)."""
    one_thread = oracle.sweeps
    oracle.sweeps = functools.partial(one_thread, n_threads=16)
    try:
        o = OracleEngine(J=J, h=h)
        o.init_replicas(R, seed=seed)
        o.set_ladder(temps)
        return run(o, R, script)
    finally:
        oracle.sweeps = one_thread


# n at the edges of the bit layout (64-bit words, 256-element segments), R with ragged replica groups (groups of 32
# or more), every W, every kind of couplings, every storage -- and with them both field sources: int8 rows with
# |J| <= 100 (8 magnitude planes) are converted on chip, everything else reads resident planes.
CASES = [
    (3, 3, 256, "f32", "pm1"), (63, 1, 512, "i8", "tern"), (64, 3, 1024, "t2", "tern"), (65, 130, 256, "f32", "a7"),
    (255, 3, 512, "i8", "a100"), (256, 130, 1024, "f32", "pm1"), (257, 1, 256, "i8", "a7"), (257, 130, 512, "f32", "a100"),
    (1000, 130, 512, "t2", "tern"), (1000, 1024, 256, "f32", "a100"), (1000, 1024, 1024, "i8", "pm1"),
    (1000, 3, 1024, "i8", "a100"), (10000, 3, 512, "f32", "pm1"), (10000, 130, 1024, "i8", "tern"),
    (10000, 1, 256, "t2", "tern"),
]


@pytest.mark.parametrize("n,R,W,storage,kind", CASES)
def test_equals_the_oracle_and_the_row_per_proposal_kernel(sg, n, R, W, storage, kind):
    J, h = couplings(n, kind, 17 + n + R), fields(n, kind, n)
    temps, seed = temps_for(n, R, kind), 1000 + n + R
    script = [1, 1] if n >= 10000 else [3, 2, 2]  # several sweeps per launch, exchange rounds between the launches
    source = "on-chip conversion" if (storage == "i8" and kind == "a100") else "resident bit-planes"
    new = engine_run(sg, J, h, R, W, storage, True, temps, seed, script, source)
    old = engine_run(sg, J, h, R, W, storage, False, temps, seed, script)
    assert_same(new, old, "row-per-proposal kernel")
    assert_same(new, oracle_run(J, h, R, temps, seed, script), "oracle")


def test_the_headline_shape_equals_the_row_per_proposal_kernel_and_itself(sg):
    """C2a's own shape (the oracle would take minutes here; it is pinned at R <= 130 above): the form against the kernel
    it replaces, and twice against itself -- the order of the entries inside a bucket differs from run to run and
    must not leak into any result."""
    n, R, W = 10000, 1024, 512
    J, h = couplings(n, "pm1", 5), fields(n, "pm1", 6)
    temps = ladder(R, 10.0, 0.1)
    a = engine_run(sg, J, h, R, W, "f32", True, temps, 4242, [2, 1], "resident bit-planes")
    b = engine_run(sg, J, h, R, W, "f32", True, temps, 4242, [2, 1], "resident bit-planes")
    c = engine_run(sg, J, h, R, W, "f32", False, temps, 4242, [2, 1])
    assert_same(a, b, "second run")
    assert_same(a, c, "row-per-proposal kernel")


@pytest.mark.parametrize("n,storage", [(PLAN_TILE, "i8"), (PLAN_TILE + 1, "i8"), (20000, "t2")])
def test_both_sides_of_the_plan_tile_bound(sg, n, storage):
    """n <= 16384 sites is one tile of the plan's LDS histogram; 16385 makes a second tile of one site."""
    R, W = 3, 1024
    J, h = couplings(n, "tern", n), fields(n, "tern", n)
    temps, seed, script = temps_for(n, R, "tern"), 77, [1, 1]
    new = engine_run(sg, J, h, R, W, storage, True, temps, seed, script, "resident bit-planes")
    assert_same(new, oracle_run(J, h, R, temps, seed, script), "oracle")


def test_a_second_set_dense_drops_the_planes(sg):
    """Stale planes are the bug to rule out: the same engine takes other couplings of the same n, then another n, then
    another storage; every run equals a fresh oracle."""
    R, W, seed = 6, 256, 31
    with sg.AnnealEngine(0) as e:
        forced(e, W)
        for n, kind, storage in [(700, "pm1", "f32"), (700, "tern", "f32"), (1300, "a7", "f32"), (1300, "pm1", "i8"),
                                 (700, "a100", "i8"), (700, "tern", "t2")]:
            J, h = couplings(n, kind, 3 * n + len(kind)), fields(n, kind, n)
            temps = temps_for(n, R, kind)
            e.set_dense(J, h, storage=storage)
            e.init_replicas(R, seed=seed)
            e.set_ladder(temps)
            got = run(e, R, [2, 2])
            assert "sweep=row-shared" in e.describe()
            assert_same(got, oracle_run(J, h, R, temps, seed, [2, 2]), (n, kind, storage))


def test_init_replicas_with_another_count_keeps_the_planes(sg):
    n, W, seed = 900, 512, 8
    J, h = couplings(n, "pm1", 1), fields(n, "pm1", 2)
    with sg.AnnealEngine(0) as e:
        forced(e, W)
        e.set_dense(J, h, storage="f32")
        for R in (5, 130, 33):
            temps = temps_for(n, R, "pm1")
            e.init_replicas(R, seed=seed + R)
            e.set_ladder(temps)
            got = run(e, R, [2, 1])
            assert_same(got, oracle_run(J, h, R, temps, seed + R, [2, 1]), R)


def test_autotune_in_mid_run_keeps_the_planes_and_the_chain(sg):
    """The autotuner's W = 256 / 512 / 1024 trials run on the planes the forced form built before it; the run goes on
    as the oracle's uninterrupted one, whatever the autotuner keeps."""
    n, R, seed = 2000, 64, 12
    J, h = couplings(n, "pm1", 9), fields(n, "pm1", 9)
    temps = ladder(R, 10.0, 0.1)
    want = oracle_run(J, h, R, temps, seed, [2, 3])
    with sg.AnnealEngine(0) as e:
        forced(e, 512)
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_ladder(temps)
        a = e.sweep(2, energy_trace=True)["energy_trace"]
        e.exchange()
        e.set_option("row_shared", 2)  # (the default: the autotuner times the form's windows and keeps the best, if any)
        e.set_option("row_shared_window", 0)
        e.autotune()
        forms = {k for k in e.autotune_table(forms=True) if k.startswith("row-shared:")}
        assert forms == {"row-shared:W256", "row-shared:W512", "row-shared:W1024"}
        b = e.sweep(3, energy_trace=True)["energy_trace"]
        got = state(e, R)
        got["trace"] = np.vstack([a, b])
    assert_same(got, want, "oracle")
