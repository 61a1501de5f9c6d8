"""The chain of the row-shared windows (rs_chain_kernel, csrc/sweep_dense_rs.hip) walks a window block by block: a block of
64 updates takes the corrections of the window's earlier accepts when it becomes current, and inside a block the
couplings of the first few accepting updates are fetched together and committed from registers for as long as the
chain's next accept is one of them.  Nothing of that may show: spins, energies, accept counters and best states are
equal -- not close -- to the CPU oracle's, at the edges of blocks and windows, on all three sources of the
correction (2-bit planes, fp32 rows, int8 rows), with a T = 0 and a T = inf replica in every run, and where an accept
changes the decisions that were pending when its coupling was fetched.  The split scan of the window plan is pinned
at its chunk edges (1024 sites) on both sides of a replica-group boundary."""
import functools
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_engine import OracleEngine  # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("inf")
# kind of couplings -> (storage, largest |J|, what last_kernel names)
SOURCES = {
    "pm1": ("f32", 1, "<float, planes=1,", "resident bit-planes"),     # the correction comes from the 2-bit planes
    "a7": ("f32", 7, "<float, planes=3,", "resident bit-planes"),      # three magnitude planes: fp32 row gathers
    "a100": ("i8", 100, "<int8_t, planes=8,", "on-chip conversion"),   # int8 row gathers
}


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


@functools.lru_cache(maxsize=None)
def problem(n, kind):
    """Symmetric integer couplings with a zero diagonal whose largest magnitude is the kind's, and fields; the fields
    of "a7" and "a100" are nowhere zero."""
    amp = SOURCES[kind][1]
    rng = np.random.RandomState(1000 * amp + n)
    if kind == "pm1":
        A = rng.randint(0, 2, (n, n)) * 2 - 1
        h = rng.randint(-1, 2, n)
    else:
        A = rng.randint(-amp, amp + 1, (n, n))
        A[0, 1] = amp
        h = rng.randint(1, 4, n) * (rng.randint(0, 2, n) * 2 - 1)
    A = np.triu(A, 1)
    return (A + A.T).astype(np.float32), h.astype(np.float32)


def temperatures(n, R, amp):
    """R >= 3: T = inf, a geometric ladder, T = 0.  R = 1: one schedule row per sweep -- inf, 0, the ladder's middle."""
    hot = 2.0 * amp * np.sqrt(n)
    if R == 1:
        return np.asarray([[INF], [0.0], [np.sqrt(hot * 0.3)]])
    return np.asarray([INF] + [hot * (0.3 / hot) ** (i / max(R - 3, 1)) for i in range(R - 2)] + [0.0])


def forced(e, W, on=True):
    e.set_option("row_shared", 1 if on else 0)
    e.set_option("row_shared_window", W)


def state(e, R, trace):
    best = [e.best(r) for r in range(R)]
    return {"trace": np.vstack(trace), "spins": np.asarray(e.spins()), "energy": np.asarray(e.energies()),
            "accepted": np.asarray(e.stats()[0]), "best_energy": np.asarray([b[0] for b in best]),
            "best_spins": np.stack([np.asarray(b[1]) for b in best])}


def three_sweeps(e, R, temps):
    """Three sweeps; with more than one replica, an exchange round after the second."""
    if R == 1:
        return state(e, R, [e.sweep(3, sched=temps, energy_trace=True)["energy_trace"]])
    e.set_ladder(temps)
    a = e.sweep(2, energy_trace=True)["energy_trace"]
    e.exchange()
    return state(e, R, [a, e.sweep(1, energy_trace=True)["energy_trace"]])


@functools.lru_cache(maxsize=None)
def oracle_three_sweeps(n, R, kind, seed):
    J, h = problem(n, kind)
    temps = temperatures(n, R, SOURCES[kind][1])
    if R == 1:
        s = oracle.init_spins(n, 1, seed)
        ref = oracle.sweeps(oracle.Problem(J=J, h=h), s, temps, 3, seed=seed)
        return {"trace": ref["energy_trace"], "spins": s, "energy": ref["energy"], "accepted": ref["n_accepted"],
                "best_energy": ref["best_energy"], "best_spins": ref["best_spins"]}
    o = OracleEngine(J=J, h=h)
    o.init_replicas(R, seed=seed)
    return three_sweeps(o, R, temps)


def engine_three_sweeps(sg, J, h, R, W, storage, temps, seed, on=True, names=()):
    from spin_glass_anneal_rl_amd.engine import last_kernel
    with sg.AnnealEngine(0) as e:
        forced(e, W, on)
        e.set_dense(J, h, storage=storage)
        e.init_replicas(R, seed=seed)
        out = three_sweeps(e, R, temps)
        if on:
            assert f"sweep=row-shared(W={W} " in e.describe(), e.describe()
            assert last_kernel().startswith("sweep_dense_rs<"), last_kernel()
            for name in names:
                assert name in last_kernel(), last_kernel()
        else:
            assert last_kernel().startswith("sweep_dense_kernel<"), last_kernel()
    return out


def assert_same(a, b, what=""):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


# ---- block and window edges, every source of the correction -----------------------------------------------------------
# n = 3 and 64 repeat sites inside a block, 130 and 300 across blocks; 65 and 130 leave a block of one or two updates;
# 1100 at W = 1024 is a window of 16 blocks and one of 76 updates with a half-empty block, at W = 256 five windows.
@pytest.mark.parametrize("R", [1, 5, 33])
@pytest.mark.parametrize("W", [256, 512, 1024])
@pytest.mark.parametrize("n", [3, 64, 65, 130, 300, 1100])
@pytest.mark.parametrize("kind", list(SOURCES))
def test_block_and_window_edges_equal_the_oracle(sg, kind, n, W, R):
    storage, amp, inst, source = SOURCES[kind]
    J, h = problem(n, kind)
    assert np.abs(J).max() == amp and (kind == "pm1" or np.all(h != 0))
    seed = 31 * n + R
    want = oracle_three_sweeps(n, R, kind, seed)
    got = engine_three_sweeps(sg, J, h, R, W, storage, temperatures(n, R, amp), seed, names=(inst, source))
    assert_same(got, want, "oracle")
    # the inputs hold what the case is about: the sweeps at T = inf accept every proposal, far more than K a block
    # (replica 0 holds the T = inf slot for the two sweeps before the exchange round; R = 1: for the first sweep)
    if R > 1:
        assert want["accepted"][0] >= 2 * n
    else:
        first = oracle.sweeps(oracle.Problem(J=J, h=h), oracle.init_spins(n, 1, seed), INF, 1, seed=seed)
        assert first["n_accepted"][0] == n


def test_equals_the_row_per_proposal_kernel_on_the_same_engine(sg):
    n, R, W, seed = 1100, 33, 1024, 5
    J, h = problem(n, "pm1")
    temps = temperatures(n, R, 1)
    from spin_glass_anneal_rl_amd.engine import last_kernel
    runs = []
    with sg.AnnealEngine(0) as e:
        for on in (True, False):
            forced(e, W, on)
            e.set_dense(J, h, storage="f32")
            e.init_replicas(R, seed=seed)
            runs.append(three_sweeps(e, R, temps))
            assert last_kernel().startswith("sweep_dense_rs<" if on else "sweep_dense_kernel<"), last_kernel()
    assert_same(runs[0], runs[1], "row-per-proposal kernel")
    assert_same(runs[0], oracle_three_sweeps(n, R, "pm1", seed), "oracle")


# ---- accepts that change the pending decisions ---------------------------------------------------------------------
# Uniform couplings J = +1 (or -1) off the diagonal, h = 0: every accept shifts every pending field by 2.
SPEC_N, SPEC_LOW_T = 130, 20.0  # (low: the mean-field transition of these couplings lies at T = n - 1)
SPEC_SEEDS = {1: 1, -1: 1}      # sign of J -> seed (chosen on the host with speculation_events below)


def uniform_couplings(n, sign):
    J = np.full((n, n), float(sign), np.float32)
    np.fill_diagonal(J, 0.0)
    return J, np.zeros(n, np.float32)


def speculation_events(sign, seed, T, replica, n_sweeps=3):
    """The oracle's chain of one replica at fixed T, replayed block by block (64 updates, cut by the end of a sweep:
    n = 130 is one window of any W).  Per block: does an update accept that rejected against the block-start spins
    (an accept that no fetch at the block's start covers), and does one reject that accepted against them (a fetched
    candidate that is dropped)?  -> list of (late accept, dropped candidate) per block."""
    n = SPEC_N
    J, h = uniform_couplings(n, sign)
    prob = oracle.Problem(J=J, h=h)
    s = oracle.init_spins(n, replica + 1, seed)[replica:replica + 1].copy()
    events = []
    for k in range(n_sweeps):
        sites = [oracle.stream_site(seed, replica, k, t, n) for t in range(n)]
        us = [oracle.stream_u(seed, replica, k, t) for t in range(n)]
        for b0 in range(0, n, 64):
            start = s[0].copy()
            late = dropped = False
            for t in range(b0, min(b0 + 64, n)):
                at_start, _ = oracle.metropolis_update(prob, start.copy(), sites[t], T, us[t])
                now, _ = oracle.metropolis_update(prob, s[0], sites[t], T, us[t])  # (in place: the chain itself)
                late |= now and not at_start
                dropped |= at_start and not now
            events.append((late, dropped))
    # the replay is the oracle's own chain
    ref = oracle.init_spins(n, replica + 1, seed)
    oracle.sweeps(prob, ref, T, n_sweeps, seed=seed)
    assert np.array_equal(ref[replica], s[0])
    return events


@pytest.mark.parametrize("W", [256, 512, 1024])
@pytest.mark.parametrize("sign", [1, -1])
def test_accepts_that_change_pending_decisions(sg, sign, W):
    n, seed = SPEC_N, SPEC_SEEDS[sign]
    temps = np.asarray([INF, 0.0, SPEC_LOW_T])
    # The inputs do what the case is about (host only).  At T = 0 the magnetisation moves one way only (J = +1: away from
    # 0, J = -1: towards 0 and no further), so pending accepts can be dropped there and no pending reject can turn:
    # the block that holds both events is the low-T replica's, the T = 0 replica's blocks hold drops.
    cold = speculation_events(sign, seed, 0.0, 1, n_sweeps=2)  # (the sweeps before the exchange round)
    low = speculation_events(sign, seed, SPEC_LOW_T, 2, n_sweeps=2)
    assert any(dropped for _, dropped in cold), (sign, seed, cold)
    assert any(late and dropped for late, dropped in low), (sign, seed, low)
    J, h = uniform_couplings(n, sign)
    o = OracleEngine(J=J, h=h)
    o.init_replicas(3, seed=seed)
    want = three_sweeps(o, 3, temps)
    got = engine_three_sweeps(sg, J, h, 3, W, "f32", temps, seed, names=("planes=1,",))
    assert_same(got, want, "oracle")


# ---- the scan of the window plan at its chunk edges ----------------------------------------------------------------
# One workgroup per (window, chunk of 1024 sites): n = 1024 is one full chunk, 1025 a second chunk of one site, 2049 a
# third; the plan groups replicas by 32 at these sizes, so R = 32 is one full group and 33 a second group of one.
@pytest.mark.parametrize("n,R,W", [(1024, 32, 256), (1024, 33, 256), (1025, 32, 256), (1025, 33, 256), (2049, 32, 256),
                                   (2049, 33, 256), (2049, 33, 1024), (1025, 33, 512)])
def test_scan_chunk_edges_equal_the_oracle(sg, n, R, W):
    J, h = problem(n, "pm1")
    seed = n + R
    got = engine_three_sweeps(sg, J, h, R, W, "f32", temperatures(n, R, 1), seed, names=("planes=1,",))
    assert_same(got, oracle_three_sweeps(n, R, "pm1", seed), "oracle")
