"""The prologue of the row-shared chain (rs_chain_kernel, csrc/sweep_dense_rs.hip): the window's base slots are loaded raw
for every lane, the gathers of h and spin follow, the conversions that wait come last, and the current block's values are
read from register vectors by the block's index.  None of it may show: spins, energies, accept counters, temperatures and
best states are equal -- not close -- to the CPU oracle's and to the row-per-proposal kernel's on the same engine, and so
are the accept counters taken before the exchange round.

Shapes: n gives last windows on both sides of 64 and 128 updates, odd and even, one-block and cut ones; W = 256, 512, 1024
are the three block counts; R = 65 runs at one replica group and at two (32 + 33: a group that starts at replica 32 and a
ragged plan slice).  Script: three sweeps in one launch, an exchange round, two more.  Every run holds a T = inf and a T = 0
slot.  Kinds, one per template axis of the chain: +-1 fp32 (sign-only planes), |J| <= 7 (three planes), int8 rows with
|J| <= 100 (rows of J itself; the per-site fields kernel, which takes one group whatever is asked), J = +-1/4 with
quarter-valued h on the binary grid, Glauber on +-1, and two field vectors over one +-1 matrix as a shard of 65 of 80
replicas whose model boundary (local replica 25) lies inside the first group.

What the chains hold is asserted on the host from the oracle's stream -- its record of every update of the three sweeps
before the exchange round (accept_trace; Glauber: the flips), which sums to the counters the engine must show there:
wherever a window has a second block, an accept in an odd block of a window (the upper half of a pair of blocks that one
Philox block per two updates would fill), and wherever n is odd (W is even: the last window's length is odd), an accept on
the last update of that window.  Under Metropolis the replica in the T = inf slot accepted all 3 n proposals."""
import functools
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_row_shared_chain_gpu as chain  # noqa: E402
from oracle_engine import OracleEngine  # noqa: E402
from test_replica_groups_gpu import assert_groups, full_state, sg  # noqa: E402,F401
from test_row_shared_tiles_gpu import assert_same, select  # noqa: E402

pytestmark = pytest.mark.gpu

NS = (3, 64, 65, 127, 128, 129, 191, 193, 300, 1100)
WS = (256, 512, 1024)
R = 65
FIRST, SECOND = 3, 2          # sweeps before and after the exchange round; the first block is one launch
SHARD = (2, 40, 15)           # "shared": M field vectors x k replicas, the shard starts at replica 15 (65 of 80)
# kind -> (couplings of test_row_shared_chain_gpu, storage, fields kernel, sign-only rows, largest |J|)
KINDS = {
    "pm1": ("pm1", "f32", "tiles", True, 1.0),
    "a7": ("a7", "f32", "tiles", False, 7.0),
    "a100-i8": ("a100", "i8", "site", None, 100.0),
    "grid": ("pm1", "f32", "tiles", True, 0.25),
    "glauber": ("pm1", "f32", "tiles", True, 1.0),
    "shared": ("pm1", "f32", "tiles", True, 1.0),
}


def tile_sites(n):
    return 24 if n <= 300 else 96


@functools.lru_cache(maxsize=None)
def problem(n, kind):
    """J, h (shared: [M, n]), the slot temperatures (shared: of all 80 replicas, one ladder per model), the seed."""
    src, _, _, _, amp = KINDS[kind]
    J, h = chain.problem(n, src)
    if kind == "grid":
        J = J * np.float32(0.25)
        h = (np.random.RandomState(n).randint(-6, 7, n) * 0.25).astype(np.float32)
    if kind == "shared":
        M, k, _ = SHARD
        h = np.stack([np.random.RandomState(90 + m + n).randint(-1, 2, n).astype(np.float32) for m in range(M)])
        return J, h, np.tile(chain.temperatures(n, k, amp), M), 4000 + n
    return J, h, chain.temperatures(n, R, amp), 4000 + n


def rule_of(kind):
    return oracle.RULE_GLAUBER if kind == "glauber" else oracle.RULE_METROPOLIS


@functools.lru_cache(maxsize=None)
def first_accepts(n, kind):
    """The oracle's record of the sweeps before the exchange round, from the initial state: accepted [R][FIRST][n]
    (shared: the shard's replicas)."""
    J, h, temps, seed = problem(n, kind)
    if kind == "shared":
        M, k, r0 = SHARD
        acc = []
        for m in range(M):
            s = oracle.init_spins(n, k, seed, replica0=m * k)
            ref = oracle.sweeps(oracle.Problem(J=np.array(J), h=np.array(h[m])), s, temps[m * k:(m + 1) * k], FIRST, seed=seed,
                                replica0=m * k, trace=True, n_threads=16)
            acc.append(ref["accept_trace"])
        return np.concatenate(acc)[r0:].reshape(R, FIRST, n).astype(bool)
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(oracle.Problem(J=np.array(J), h=np.array(h)), s, temps, FIRST, rule=rule_of(kind), seed=seed, trace=True,
                        n_threads=16)
    return ref["accept_trace"].reshape(R, FIRST, n).astype(bool)


@functools.lru_cache(maxsize=None)
def oracle_run(n, kind):
    """-> (the state the script leaves, with the accept counters before the exchange round as "accepted_first"; the
    energies of every replica before the exchange round)."""
    J, h, temps, seed = problem(n, kind)
    plain = oracle.sweeps
    oracle.sweeps = functools.partial(plain, n_threads=16, rule=rule_of(kind))
    try:
        if kind == "shared":
            M, k, r0 = SHARD
            os_ = [OracleEngine(J=np.array(J), h=np.array(h[m])) for m in range(M)]
            for m, o in enumerate(os_):
                o.init_replicas(k, seed=seed, R_global=M * k, replica0=m * k)
                o.set_ladder(temps, n_ladders=M)
                o.sweep(FIRST)
            mid = np.concatenate([o.energies() for o in os_])
            first = np.concatenate([o.stats()[0] for o in os_])[r0:]
            for o in os_:
                o.exchange()  # (whole ladders on each: decided from its own energies)
                o.sweep(SECOND)
            parts = [full_state(o, k) for o in os_]
            return dict({key: np.concatenate([p[key] for p in parts])[r0:] for key in parts[0]}, accepted_first=first), mid
        o = OracleEngine(J=np.array(J), h=np.array(h))
        o.init_replicas(R, seed=seed)
        o.set_ladder(temps)
        o.sweep(FIRST)
        mid, first = o.energies(), o.stats()[0]
        o.exchange()
        o.sweep(SECOND)
        return dict(full_state(o, R), accepted_first=first), mid
    finally:
        oracle.sweeps = plain


def engine_run(m, n, kind, W, G, rows=False):
    _, storage, fields, ones, _ = KINDS[kind]
    J, h, temps, seed = problem(n, kind)
    grid = 1 if kind == "grid" else 0
    with m.AnnealEngine(0) as e:
        if rows:
            select(e, "rows", 1024, grid=grid)
        else:
            select(e, fields, W, tile_sites(n) if fields == "tiles" else 0, grid=grid)
            e.set_replica_groups(G)
        e.set_tuning(sweeps_per_launch=FIRST)
        if kind == "glauber":
            e.set_update_rule(m._native.RULE_GLAUBER)
        if kind == "shared":
            M, k, r0 = SHARD
            e.set_dense_shared(J, h, storage=storage)
            e.init_replicas(R, seed=seed, R_global=M * k, replica0=r0)
            e.set_ladder(temps, n_ladders=M)
        else:
            e.set_dense(J, h, storage=storage)
            e.init_replicas(R, seed=seed)
            e.set_ladder(temps)
        e.sweep(FIRST)
        first = np.asarray(e.stats()[0]).copy()
        kernel = e.last_kernel()
        if rows:
            assert kernel.startswith("sweep_dense_kernel<"), kernel
        else:
            assert kernel.startswith("sweep_dense_rs<") and f"sweep=row-shared(W={W} " in e.describe(), (kernel, e.describe())
            if grid:
                assert "grid=2^-2>" in kernel, kernel
            if fields == "tiles":
                assert_groups(e, R, G, tile_sites(n), ones)
            else:
                assert "on-chip conversion" in kernel and "<int8_t, planes=8," in kernel and "groups=" not in kernel, kernel
        if kind == "shared":
            e.exchange(energies_global=oracle_run(n, kind)[1])  # (a shard: the round is decided from every replica's energy)
        else:
            e.exchange()
        e.sweep(SECOND)
        return dict(full_state(e, R), accepted_first=first)


@functools.lru_cache(maxsize=None)
def rows_run(n, kind):
    """The row-per-proposal kernel of the same engine."""
    import spin_glass_anneal_rl_amd as m
    return engine_run(m, n, kind, 1024, 1, rows=True)


def test_the_shapes_hold_both_halves_of_a_pass_and_an_odd_last_window():
    lasts = {(n, W): n - (-(-n // W) - 1) * W for n in NS for W in WS}
    assert any(c % 2 for c in lasts.values()) and any(c % 2 == 0 for c in lasts.values())
    assert any(c < 64 for c in lasts.values()) and any(64 < c < 128 for c in lasts.values()) and any(c > 128 for c in lasts.values())
    assert {64, 128} <= set(lasts.values()) and {65, 127, 129, 191, 193} <= set(lasts.values())
    assert any(-(-c // 64) % 2 for c in lasts.values())  # an odd number of blocks against whole passes
    assert (1100, 256) in lasts and lasts[(1100, 256)] == 76 and lasts[(1100, 1024)] == 76


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_prologue_equals_the_oracle_and_the_row_kernel(sg, kind, n, W, G):  # noqa: F811
    want, _ = oracle_run(n, kind)
    acc = first_accepts(n, kind)  # [R][FIRST][n], the oracle's own chain: it sums to the counters before the exchange round
    assert np.array_equal(acc.sum(axis=(1, 2)), want["accepted_first"])
    t = np.arange(n)
    odd_block = ((t % W) // 64) % 2 == 1
    if odd_block.any():
        assert acc[:, :, odd_block].any(), "no accept in an odd block of a window"
    if n % 2:
        assert acc[:, :, n - 1].any(), "no accept on the last update of the odd-length last window"
    if kind != "glauber":
        # the replica in the T = inf slot (shared: the second model's first, local 25) accepted every proposal
        hot = SHARD[1] - SHARD[2] if kind == "shared" else 0
        assert problem(n, kind)[2][SHARD[1] if kind == "shared" else 0] == chain.INF
        assert want["accepted_first"][hot] == FIRST * n and acc[hot].all()
    got = engine_run(sg, n, kind, W, G)
    assert_same(got, want, "oracle")
    assert_same(got, rows_run(n, kind), "row-per-proposal kernel")
