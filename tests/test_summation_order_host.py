"""The canonical fp64 summation order, pinned on the CPU (no GPU needed).

For every run tests/test_summation_order_gpu.py compares with the oracle (shared builders and seeds, tests/canonical_sum.py):

  * the oracle's traced run equals, bit for bit, a replay in Python that forms every proposed row sum with the
    independent reference of tests/canonical_sum.py -- decisions, dE records, local fields, final spins, counters;
  * the SENSITIVITY CONDITION, a condition on the inputs: under every decoy order that applies to the shape, at least
    25 % of the proposals on probe sites get another fp32 row sum than under the canonical order, so a kernel that
    summed in that order would fail the bitwise comparison of dE records and local fields;
  * production runs (no per-update records) can show the order through decisions only: the run replayed under the
    left-to-right decoy, and under the other tree, must reach a differing accept decision within the sweeps the GPU
    case runs.

Every comparison is on bits; the one number is the 25 % floor.
"""
import numpy as np
import pytest

import canonical_sum as cs
import oracle

FLOOR = 0.25
BLOCK = 256


def stream(cfg, r):
    """Sites and uniforms of replica r, one per proposal."""
    n, per = cfg["prob"].n, cfg["ns"] * cfg["prob"].n
    if cfg["kind"] == "replay":
        return cfg["site"][r], cfg["u"][r]
    if cfg["kind"] == "sequential":
        return np.tile(np.arange(n, dtype=np.int32), cfg["ns"]), cfg["u"][r]
    site = np.asarray([oracle.stream_site(cfg["seed"], r, k, t, n) for k in range(cfg["ns"]) for t in range(n)], np.int32)
    u = np.asarray([oracle.stream_u(cfg["seed"], r, k, t) for k in range(cfg["ns"]) for t in range(n)], np.float32)
    assert site.size == per
    return site, u


def replay(cfg, ref, decoys, check_fields):
    """Walk the oracle's run with canonical_sum row sums.  Returns {decoy: share of probe proposals whose fp32 row sum
    differs} and the index (replica, proposal) of the first accept decision the left-to-right order changes."""
    prob, rule = cfg["prob"], cfg["rule"]
    op = prob.oracle_problem()
    is_probe = np.zeros(prob.n, bool)
    is_probe[prob.probes] = True
    differ = {d: 0 for d in decoys}
    n_probe_proposals, first_flip = 0, {d: None for d in decoys}
    for r in range(cfg["R"]):
        site, u = stream(cfg, r)
        s = cfg["s0"][r].copy()
        T = float(cfg["temps"][r])
        acc_ref = ref["accept_trace"][r].astype(bool)
        for b0 in range(0, site.size, BLOCK):
            sl = slice(b0, min(site.size, b0 + BLOCK))
            st, B = site[sl].astype(np.int64), sl.stop - sl.start
            # the spins before each proposal IF the oracle's decisions are the replay's: checked right below, so the
            # first proposal's state is right, hence its decision, hence the second one's state, and so on
            S = np.empty((B, prob.n), np.int8)
            for k in range(B):
                S[k] = s
                if acc_ref[b0 + k]:
                    s[st[k]] = -s[st[k]]
            s_i = S[np.arange(B), st].astype(np.float64)
            P = prob.row_products(st, S)
            total = cs.dense_sum64 if prob.J is not None else cs.csr_sum64
            dot = cs.f32(total(P)).astype(np.float64)
            field = dot + prob.h[st].astype(np.float64)
            acc, rec = cs.decide(rule, s_i, field, T, u[sl])
            assert np.array_equal(acc, acc_ref[sl]), (cfg["name"], r, b0, "accept decisions")
            assert np.array_equal(rec, ref["dE_trace"][r][sl]), (cfg["name"], r, b0, "dE records")
            if check_fields:
                got = [oracle.local_field(op, S[k], int(st[k])) for k in range(B)]
                assert np.array_equal(field, got), (cfg["name"], r, b0, "local fields")
            pr = is_probe[st]
            n_probe_proposals += int(pr.sum())
            for d in decoys:
                dot_d = cs.f32(total(P, d)).astype(np.float64)
                differ[d] += int(np.sum((dot_d != dot) & pr))
                if first_flip[d] is None:
                    cand = np.nonzero((dot_d != dot) & pr)[0]
                    acc_d, _ = cs.decide(rule, s_i[cand], dot_d[cand] + prob.h[st[cand]].astype(np.float64), T, u[sl][cand])
                    if np.any(acc_d != acc[cand]):
                        first_flip[d] = (r, b0 + int(cand[np.nonzero(acc_d != acc[cand])[0][0]]))
        assert np.array_equal(s, ref["spins"][r]), (cfg["name"], r, "final spins")
        assert int(acc_ref.sum()) == int(ref["n_accepted"][r])
        assert np.array_equal(s[prob.ballast], prob.ballast_spin[prob.ballast]), (cfg["name"], r, "a ballast spin flipped")
    return {d: differ[d] / max(1, n_probe_proposals) for d in decoys}, first_flip


@pytest.mark.parametrize("name", list(cs.RUNS))
def test_oracle_follows_the_canonical_order_and_the_inputs_show_it(name):
    cfg = cs.run_setup(name)
    prob = cfg["prob"]
    production = cfg["kind"] == "production"
    ref = cs.oracle_run(cfg)
    applicable = {d: why for d, why in prob.decoys().items()}
    # production runs show the order through decisions only: the left-to-right order and the other tree (the rows
    # kernel's kind of mistake: lanes folded in another grouping) must each change one within the run
    decoys = ["left-to-right", "far-tree"] if production else [d for d, why in applicable.items() if why is None]
    assert "left-to-right" in decoys and len(decoys) >= 2
    share, first_flip = replay(cfg, ref, decoys, check_fields=not production)
    for d, why in applicable.items():
        if why is not None:
            print(f"{name}: decoy {d} not applicable: {why}")
    for d in decoys:
        print(f"{name}: decoy {d}: {100.0 * share[d]:.1f} % of the probe proposals get another fp32 row sum")
    for d in decoys:
        assert share[d] >= FLOOR, (name, d, share[d])
    if production:
        for d in decoys:
            print(f"{name}: first accept decision changed by the {d} order: (replica, proposal) = {first_flip[d]} "
                  f"of {cfg['R']} x {cfg['ns'] * prob.n}")
            assert first_flip[d] is not None, (name, d, "no decision in this run depends on the order: lengthen it")


@pytest.mark.parametrize("key", ["d700", "d2501", "c64", "c1200"])
def test_reference_agrees_with_the_oracle_on_single_rows(key):
    """local_field on every probe row of the unpinned problems, and dense_row_sum / csr_row_sum as the GPU tests call them."""
    prob = cs.problem(key, False)
    op = prob.oracle_problem()
    s = prob.s0(1, 7)[0]
    sites = prob.probes
    want = prob.row_sums(sites, np.repeat(s[None, :], len(sites), 0)) + prob.h[sites].astype(np.float64)
    assert np.array_equal(want, [oracle.local_field(op, s, int(i)) for i in sites])
    for i in sites[:16]:
        if prob.J is not None:
            one = cs.dense_row_sum(prob.J[i], s)
        else:
            rp = prob.csr[0]
            one = cs.csr_row_sum(prob.csr[2][rp[i]:rp[i + 1]], prob.csr[1][rp[i]:rp[i + 1]], s)
        assert float(one) + float(prob.h[i]) == oracle.local_field(op, s, int(i))


@pytest.mark.parametrize("kind,n", [("dense", 600), ("dense", 1100), ("dense", 2600), ("dense", 4400), ("csr", 600),
                                    ("csr", 400)])
def test_quad_problem_energies_show_every_order(kind, n):
    """The problems of the GPU energy and Wolff cases: the reference's row sums are the oracle's, and EVERY applicable
    decoy -- the other tree and the super-chunks grouped by wave among them -- changes at least a quarter of the row
    sums and moves the from-scratch energy E = -1/2 fp32(X) - fp32(Y) of every spin vector tried."""
    prob = cs.quad_problem(n, 31, as_csr=(kind == "csr"))
    op = prob.oracle_problem()
    S = cs.quad_spins(n, 3, 900 + n)
    sites = np.arange(0, n, max(1, n // 256))
    decoys = [d for d, why in prob.decoys().items() if why is None]
    assert len(decoys) >= 3 and (n <= 2048 or "by-wave-2" in decoys or kind == "csr")
    for s in S:
        rep = np.repeat(s[None, :], len(sites), 0)
        mv = prob.row_sums(sites, rep)
        assert np.array_equal(mv + prob.h[sites].astype(np.float64), [oracle.local_field(op, s, int(i)) for i in sites])
        E = cs.chain_energy(prob, s)
        for d in decoys:
            share = float(np.mean(prob.row_sums(sites, rep, d) != mv))
            Ed = cs.chain_energy(prob, s, d)
            print(f"{prob.name}: decoy {d}: {100.0 * share:.0f} % of the row sums differ, E {E!r} -> {Ed!r}")
            assert share >= FLOOR and Ed != E, (prob.name, d, share, E, Ed)


def test_gaussian_inputs_do_not_show_the_order():
    """The record of the gap: on randn couplings alone no decoy changes an fp32 row sum (printed, not asserted)."""
    prob = cs.gaussian_problem(2500, 1)
    s = prob.s0(1, 5)[0]
    sites = np.arange(400)
    S = np.repeat(s[None, :], len(sites), 0)
    can = prob.row_sums(sites, S)
    for d in cs.DENSE_DECOYS:
        print(f"randn-n2500: decoy {d}: {100.0 * np.mean(prob.row_sums(sites, S, d) != can):.1f} % of 400 rows differ")
