"""The oracle at the ends of the temperature range (no GPU): T = 0 accepts a move iff dE <= 0, and replica
exchange follows the reference's min(1.0, np.exp(x)), which swaps when x is NaN (T = 0 slots: inf * 0, inf - inf);
the operator form's rand < exp(x) does not."""
import numpy as np
import pytest

import oracle

INF = float("inf")


def problems():
    rng = np.random.RandomState(3)
    n = 150
    J = np.triu(rng.randint(-2, 3, (n, n)) * (rng.rand(n, n) < 0.2), 1).astype(np.float32)
    J = J + J.T
    h = rng.randint(-3, 4, n).astype(np.float32)
    rowptr = np.concatenate([[0], np.cumsum((J != 0).sum(1))]).astype(np.int32)
    col = np.concatenate([np.nonzero(J[i])[0] for i in range(n)]).astype(np.int32)
    val = np.concatenate([J[i][J[i] != 0] for i in range(n)]).astype(np.float32)
    return {"dense": oracle.Problem(J=J, h=h), "csr": oracle.Problem(csr=(rowptr, col, val), h=h / 2)}


@pytest.mark.parametrize("kind", ["dense", "csr"])
@pytest.mark.parametrize("arith", [oracle.ARITH_F64, oracle.ARITH_F32])
def test_oracle_zero_temperature_equals_tiny_temperature(kind, arith):
    """Integer (or half-integer) problems: every uphill move is at least 1, exp(-1 / 1e-10) is 0 in fp32, so
    T = 0 and the denormal / tiny temperatures walk the T = 1e-10 chain; a T = 0 replica's energy never rises."""
    prob = problems()[kind]
    R, ns, seed = 6, 10, 17
    cold = np.asarray([0.0, 5e-324, 1e-300, 0.0, 3.0, INF])
    tiny = np.where(cold < 1e-10, 1e-10, cold)
    runs = []
    for temps in (cold, tiny):
        s = oracle.init_spins(prob.n, R, seed)
        ref = oracle.sweeps(prob, s, temps, ns, arith=arith, seed=seed)
        runs.append((s, ref))
    (s0, a), (s1, b) = runs
    assert np.array_equal(s0, s1)
    for key in ("energy_trace", "n_accepted", "best_energy", "best_spins"):
        assert np.array_equal(a[key], b[key]), key
    start = np.asarray([oracle.energy(prob, s) for s in oracle.init_spins(prob.n, R, seed)])
    trace = np.vstack([start[None, :], a["energy_trace"]])
    for r in np.nonzero(cold == 0.0)[0]:
        assert np.all(np.diff(trace[:, r]) <= 0), r
    assert a["n_accepted"][R - 1] == ns * prob.n      # T = inf accepts every proposal


def test_oracle_sweep_schedule_reaching_zero_never_rises_at_zero():
    prob = problems()["dense"]
    R, ns, seed = 4, 12, 5
    sched = np.outer(np.maximum(0.0, 1.0 - np.arange(ns) / 5.0), [6.0, 3.0, 1.0, 0.5])
    s = oracle.init_spins(prob.n, R, seed)
    ref = oracle.sweeps(prob, s, sched, ns, seed=seed)
    cold = ref["energy_trace"][6:]                     # sweeps 6.. run at exactly 0
    assert np.all(np.diff(cold, axis=0) <= 0)


@pytest.mark.parametrize("temps", [[1.0, 0.0], [0.0, 0.0], [0.0, 5e-324], [INF, INF], [INF, 2.0]])
def test_oracle_exchange_swaps_on_nan(temps):
    """Equal energies: x = (beta_j - beta_i) * 0 is 0 or NaN; min(1.0, np.exp(x)) is 1 either way."""
    energies = np.asarray([-7.0, -7.0])
    for u in (0.0, 0.5, 1.0 - 2.0 ** -53):
        slot = np.arange(2, dtype=np.int32)
        att, acc = np.zeros(2, np.int64), np.zeros(2, np.int64)
        assert oracle.pt_exchange_round(temps, energies, slot, start=0, u=[u], attempts=att, accepts=acc) == 1
        assert list(slot) == [1, 0] and att[0] == acc[0] == 1
        slot = np.arange(2, dtype=np.int32)
        assert oracle.pt_exchange_pairs(temps, energies, slot, [(0, 1)], u=[u]) == 1
        assert list(slot) == [1, 0]


def test_oracle_exchange_at_zero_slots_with_different_energies():
    """A T = 0 slot next to a warmer one: x = +-inf, a certain swap towards the lower energy at T = 0 and none
    away from it."""
    slot = np.arange(2, dtype=np.int32)
    assert oracle.pt_exchange_round([1.0, 0.0], [-3.0, -5.0], slot, start=0, u=[0.0]) == 0
    assert oracle.pt_exchange_round([1.0, 0.0], [-5.0, -3.0], slot, start=0, u=[0.999]) == 1


def test_oracle_operator_exchange_keeps_no_swap_on_nan():
    n = 8
    spins = oracle.init_spins(n, 4, 3)
    for temps in ([1.0, 0.0, 0.0, 2.0], [INF, 0.0, 0.0, 1.0]):
        s, e = spins.copy(), np.full(4, -4.0, np.float32)
        assert oracle.pt_exchange_operator(s, e, np.asarray(temps, np.float32), np.zeros(3, np.float32)) == 0
        assert np.array_equal(s, spins)
