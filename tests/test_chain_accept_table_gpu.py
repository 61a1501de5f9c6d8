"""The accept table of the row-shared chain (rs_chain_kernel, csrc/sweep_dense_rs.hip): a wave tabulates the Metropolis
probabilities of its temperature in LDS once per window, answers "false" beyond a table that ends in zeros, and evaluates
a q beyond a table that does not per lane.  Nothing of that may show: spins, energies, accept counters and best states are
equal -- not close -- to the CPU oracle's, on all three sources of the correction, with ladders that hold T = 0, T = inf, a
temperature on each side of 1023 / 52 (the colder one's table ends below the cap) and one far above.  That each run
holds the decisions it is about is asserted on the host, from a replay of the oracle's chain."""
import functools
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept_table_rule as at  # noqa: E402
from oracle_engine import OracleEngine  # noqa: E402
from test_row_shared_chain_gpu import SOURCES, assert_same, engine_three_sweeps, problem, sg, three_sweeps  # noqa: E402,F401

pytestmark = pytest.mark.gpu

INF = float("inf")
FAR, ABOVE, BELOW = 2000.0, 19.7, 19.6  # 1023 / 52 = 19.67...: at 19.6 the table ends at q = 1021, in zeros


def ladder(R):
    """inf, far above the cap, the two sides of 1023 / 52, (R = 33: a geometric ladder 12 -> 0.3,) 0."""
    mid = [12.0 * (0.3 / 12.0) ** (i / (R - 6)) for i in range(R - 5)] if R > 5 else []
    return np.asarray([INF, FAR, ABOVE, BELOW] + mid + [0.0])


def table_m(J, h):
    return int((np.abs(J).sum(1) + np.abs(h)).max())


@functools.lru_cache(maxsize=None)
def decisions(kind, n, R, seed):
    """The oracle's chain of the two sweeps before the exchange round, replayed update by update: every uphill decision
    as (how the table form answers it, its probability, accepted) -> a set."""
    J, h = problem(n, kind)
    temps, m = ladder(R), table_m(J, h)
    s = oracle.init_spins(n, R, seed)
    seen = set()
    prob = functools.lru_cache(maxsize=None)(at.probability)
    for r in range(R):
        T, sr = float(temps[r]), s[r].astype(np.float32)
        for k in range(2):
            for t in range(n):
                i, u = oracle.stream_site(seed, r, k, t, n), oracle.stream_u(seed, r, k, t)
                q = int(sr[i] * (J[i] @ sr + h[i]))
                acc, how = at.tabled(q, u, T, m)
                if q > 0:
                    p = prob(q, T)
                    seen.add((how, "between" if 0.0 < p < 1.0 else "zero" if p == 0.0 else "one", acc))
                if acc:
                    sr[i] = -sr[i]
        s[r] = sr.astype(np.int8)
    # the replay is the oracle's own chain
    ref = oracle.init_spins(n, R, seed)
    oracle.sweeps(oracle.Problem(J=J, h=h), ref, temps, 2, seed=seed)
    assert np.array_equal(ref, s)
    return frozenset(seen)


@functools.lru_cache(maxsize=None)
def oracle_run(kind, n, R, seed):
    J, h = problem(n, kind)
    o = OracleEngine(J=J, h=h)
    o.init_replicas(R, seed=seed)
    return three_sweeps(o, R, ladder(R))


@pytest.mark.parametrize("R", [5, 33])
@pytest.mark.parametrize("W", [256, 1024])
@pytest.mark.parametrize("n", [130, 300, 1100])
@pytest.mark.parametrize("kind", list(SOURCES))
def test_table_decisions_equal_the_oracle(sg, kind, n, W, R):  # noqa: F811
    storage, amp, inst, source = SOURCES[kind]
    J, h = problem(n, kind)
    seed = 17 * n + R
    # what the run is about (host only): decisions answered by an entry strictly between 0 and 1, accepted and rejected,
    # and decisions answered "false" beyond a table that ends in zeros; the |J| <= 100 rows, whose fields reach past the
    # cap, also hold decisions that a lane evaluates beyond the table, accepted and rejected, with 0 < p < 1
    seen = decisions(kind, n, R, seed)
    assert ("table", "between", True) in seen and ("table", "between", False) in seen, sorted(seen)
    assert ("zero", "zero", False) in seen, sorted(seen)
    assert not any(how == "zero" and what != "zero" for how, what, _ in seen)
    if kind == "a100":
        assert table_m(J, h) > at.MAX
        assert ("lane", "between", True) in seen and ("lane", "between", False) in seen, sorted(seen)
        assert ("lane", "one", True) in seen  # (T = inf beyond the cap)
    got = engine_three_sweeps(sg, J, h, R, W, storage, ladder(R), seed, names=(inst, source))
    assert_same(got, oracle_run(kind, n, R, seed), "oracle")
