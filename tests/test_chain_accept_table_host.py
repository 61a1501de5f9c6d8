"""The accept table of the row-shared chain (csrc/sweep_dense_rs.hip, rs_accept_tabled), what holds without a GPU: the
size rule rs_accept_table_entries (tests/c_abi/rs_accept_table_rule.cpp over sga_kernels.h) against the rule written out
in accept_table_rule.py, and -- with the oracle's expf -- that the table form decides as rs_accept's direct expression does,
for every q up to min(table_m, 2200) at temperatures on both sides of every edge of the rule: 0, 1e-30, k / 52 and its two
fp64 neighbours for k = 1, 2, 1021, 1022, 1023, 1e6 and inf."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept_table_rule as at  # noqa: E402

INF = float("inf")
TABLE_MS = (1, 520, 1023, 1024, 9999)


def temperatures():
    ts = [0.0, 1e-30]
    for k in (1, 2, 1021, 1022, 1023):
        t = k / 52.0
        ts += [float(np.nextafter(t, -INF)), t, float(np.nextafter(t, INF))]
    return ts + [1e6, INF]


QUERIES = [(T, m) for T in temperatures() for m in TABLE_MS]


def uniforms(p):
    """0, 2^-24, 1 - 2^-24, and the 24-bit uniforms just below and at or above p."""
    k = int(np.ceil(np.float64(p) * 2.0 ** 24))
    return sorted({0.0, 2.0 ** -24, 1.0 - 2.0 ** -24} | {j * 2.0 ** -24 for j in (k - 1, k) if 0 <= j < 2 ** 24})


def check(exe):
    head, got = at.ask(exe, QUERIES)
    assert head == f"max={at.MAX}"
    for (T, m), (Q, z) in zip(QUERIES, got):
        assert (Q, z) == (at.entries(T, m), at.zero_from(T)), (T, m)
        assert 0 <= Q <= min(m, at.MAX)
    # T = 0 gives the minimum; T = inf and any T above 1023 / 52 the cap
    by = dict(zip(QUERIES, got))
    assert [by[(0.0, m)][0] for m in TABLE_MS] == [1, 2, 2, 2, 2]
    for T in (float(np.nextafter(1023 / 52.0, INF)), 1e6, INF):
        assert [by[(T, m)] for m in TABLE_MS] == [(1, at.NO_BOUND), (520, at.NO_BOUND), (1023, at.NO_BOUND), (1023, at.NO_BOUND), (1023, at.NO_BOUND)]
    assert by[(1022 / 52.0, 9999)] == (1023, 1024)  # (floor(52 T) + 2 = 1024: the cap cuts it, beyond it the lanes evaluate)
    assert by[(1.0 / 52.0, 9999)] == (3, 3) and by[(float(np.nextafter(1.0 / 52.0, -INF)), 9999)] == (2, 2)


def test_rule(tmp_path):
    check(at.build(tmp_path))


def test_rule_under_sanitizers(tmp_path):
    """The same program, stand-alone, with the address and undefined-behaviour sanitizers on its host code."""
    check(at.build(tmp_path, flags=("-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all")))


def test_table_form_decides_as_the_direct_expression():
    prob = functools.lru_cache(maxsize=None)(at.probability)
    how_seen = set()
    for T, m in QUERIES:
        Q, z = at.entries(T, m), at.zero_from(T)
        for q in range(0, min(m, 2200) + 1):
            p = prob(q, T) if q >= 1 else 1.0
            for u in uniforms(p):
                want = True if q <= 0 else u < p  # (q <= table_m: rs_accept's table branch, the direct expression)
                assert at.direct(q, u, T, m) == want
                got, how = at.tabled(q, u, T, m)
                assert got == want, (T, m, q, u, how, p)
                how_seen.add(how)
            if q > Q and Q == z:
                assert p == 0.0, (T, m, q, p)  # "false beyond Q": the entry would be exactly zero
        # the last nonzero entry never lies beyond floor(52 T)
        if z != at.NO_BOUND and T > 0:
            assert all(prob(q, T) == 0.0 for q in range(int(52.0 * T) + 1, min(m, 2200) + 1)), (T, m)
    assert how_seen == {"down", "table", "zero", "lane"}
