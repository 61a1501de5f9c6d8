"""Every sweep form and every exchange at the ends of the temperature range: T = 0 (accept iff dE <= 0),
denormal and tiny T, huge T and T = inf (accept every Metropolis proposal), in one launch.

include/sga.h promises that no form option changes a result.  Each case here forces one form, checks that the
form actually ran (last_kernel / describe), and compares it bit for bit with the oracle; three properties that do
not rest on the oracle's own T = 0 arithmetic are checked besides: a T = 0 chain equals the T = 1e-10 chain on
integer problems, a T = 0 replica's energy never rises, and a T = inf Metropolis replica accepts every proposal.
"""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

INF = float("inf")
# slot values: exactly 0, the smallest denormal, a tiny normal, the annealers' floor, two ordinary values, huge, inf
EDGE = [0.0, 5e-324, 1e-300, 1e-10, 0.5, 3.0, 1e30, INF]


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def edge_temps(R, scale=1.0):
    """R >= 8 replica temperatures cycling through EDGE; the two ordinary values scaled to the problem."""
    t = [v * scale if v in (0.5, 3.0) else v for v in EDGE]
    return np.asarray([t[r % len(t)] for r in range(R)], np.float64)


def cooling_sched(ns, R, scale=1.0):
    """[ns, R]: replica 0 at inf, replica R-1 at exactly 0, the others cooling from hot to exactly 0.0 at 60 % of
    the call."""
    k = np.arange(ns, dtype=np.float64)[:, None]
    hot = 3.0 * scale * (1.0 + np.arange(R, dtype=np.float64)[None, :])
    s = hot * np.maximum(0.0, 1.0 - k / (0.6 * (ns - 1)))
    s[:, 0], s[:, R - 1] = INF, 0.0
    assert np.all(s[-1, 1:] == 0.0)
    return np.ascontiguousarray(s)


def pm1(n, seed):
    rng = np.random.RandomState(seed)
    J = np.triu(rng.randint(0, 2, (n, n)) * 2 - 1, 1).astype(np.float32)
    return J + J.T


def int_couplings(n, seed, amp, density=1.0):
    rng = np.random.RandomState(seed)
    J = np.triu(rng.randint(-amp, amp + 1, (n, n)) * (rng.rand(n, n) < density), 1).astype(np.float32)
    return J + J.T


def csr_of(J):
    n = J.shape[0]
    rowptr = np.concatenate([[0], np.cumsum((J != 0).sum(1))]).astype(np.int32)
    col = np.concatenate([np.nonzero(J[i])[0] for i in range(n)] + [np.zeros(0, int)]).astype(np.int32)
    val = np.concatenate([J[i][J[i] != 0] for i in range(n)] + [np.zeros(0)]).astype(np.float32)
    return rowptr, col, val


def sparse_int(n, deg, amp, seed):
    rng = np.random.RandomState(seed)
    J = np.zeros((n, n), np.float32)
    for i in range(n):
        for j in rng.choice(n, max(1, deg // 2), replace=False):
            if i != j:
                J[i, j] = J[j, i] = float(rng.choice([v for v in range(-amp, amp + 1) if v != 0]))
    return J


def check_properties(ref, e0, temps, rule, acc_att, label):
    """The oracle-independent checks on one run at fixed per-replica temperatures."""
    trace = np.vstack([e0[None, :], ref["energy_trace"]])
    for r, T in enumerate(temps):
        if T == 0.0 and rule in (0, 1, 2):
            assert np.all(np.diff(trace[:, r]) <= 0), (label, "T = 0 replica's energy rose", r, trace[:, r])
        if T == INF and rule == 0:
            assert acc_att[0][r] == acc_att[1][r] > 0, (label, "T = inf replica rejected a proposal", r, acc_att)


def run_form(sg, prob, setup, R, ns, seed, want, temps=None, sched=None, rule=0, site_mode=0, arith=0,
             replay_u=None, recompute=False, exact=True, label=""):
    """One forced form against the oracle: which kernel ran, then trace, spins, energies, best states and
    acceptance counters bit for bit."""
    n = prob.n
    s = oracle.init_spins(n, R, seed)
    e0 = np.asarray([oracle.energy(prob, s[r]) for r in range(R)])
    ref = oracle.sweeps(prob, s, sched if sched is not None else temps, ns, rule=rule, site_mode=site_mode,
                        arith=arith, replay_u=replay_u, seed=seed, recompute_energy=recompute, n_threads=8)
    with sg.AnnealEngine(0) as e:
        setup(e)
        e.set_update_rule(rule)
        e.init_replicas(R, seed=seed)
        e.set_temperatures(temps if temps is not None else np.ones(R))
        out = e.sweep(ns, site_mode=site_mode, arith=arith, sched=sched, replay_u=replay_u, energy_trace=True)
        k, d = e.last_kernel(), e.describe()
        got = dict(trace=out["energy_trace"], spins=e.spins(), energy=e.energies(), stats=e.stats(),
                   best=[e.best(r) for r in range(R)])
    tag = (label, k, d)
    assert want(k, d), tag
    if exact:
        assert np.array_equal(got["trace"], ref["energy_trace"]), tag
        assert np.array_equal(got["energy"], ref["energy"]), tag
    else:
        assert np.allclose(got["trace"], ref["energy_trace"], rtol=1e-6, atol=1e-5), tag
    assert np.array_equal(got["spins"], s), tag
    assert np.array_equal(got["stats"][0], ref["n_accepted"]), tag
    for r in range(R):
        be, bs, _ = got["best"][r]
        if exact:
            assert be == ref["best_energy"][r], (tag, r)
        assert np.array_equal(bs, ref["best_spins"][r]), (tag, r)
    if sched is None:
        check_properties(ref, e0, temps, rule, got["stats"], tag)
    else:  # the replica held at 0 throughout, and the one at inf
        check_properties(ref, e0, [INF] + [np.nan] * (R - 2) + [0.0], rule, got["stats"], tag)
    return got


def both_temperature_kinds(sg, prob, setup, R, seed, want, scale=1.0, ns=6, ns_sched=20, **kw):
    """Fixed edge temperatures, then a schedule that cools to exactly 0 inside the call."""
    run_form(sg, prob, setup, R, ns, seed, want, temps=edge_temps(R, scale), **kw)
    run_form(sg, prob, setup, R, ns_sched, seed + 1, want, sched=cooling_sched(ns_sched, R, scale), **kw)


# ----------------------------------------------------------------------------- dense, row per proposal
@pytest.mark.parametrize("storage", ["f32", "i8", "t2"])
@pytest.mark.parametrize("look", [True, False])
def test_dense_streaming_forms_at_edges(sg, storage, look):
    n, R = 256, 8
    J = pm1(n, 3)
    h = np.random.RandomState(4).randint(-1, 2, n).astype(np.float32)

    def setup(e):
        e.set_options({} if look else {"look_ahead": 0})
        e.set_dense(J, h, storage=storage)

    def want(k, d):
        la = "look_ahead=4" in d or "look_ahead=2" in d
        return k.startswith("sweep_dense_kernel") and f"storage={storage}" in d and la == look
    both_temperature_kinds(sg, oracle.Problem(J=J, h=h), setup, R, 11, want, scale=np.sqrt(n))


@pytest.mark.parametrize("rule", [1, 2])
def test_dense_and_csr_glauber_and_heat_bath_at_edges(sg, rule):
    n, R = 200, 8
    J = int_couplings(n, 5, 2, density=0.1)
    h = np.random.RandomState(5).randint(-2, 3, n).astype(np.float32)
    prob = oracle.Problem(J=J, h=h)
    both_temperature_kinds(sg, prob, lambda e: (e.set_options(sparse_route=0), e.set_dense(J, h, storage="f32")), R, 21 + rule,
                           lambda k, d: k.startswith("sweep_dense_kernel") and "storage=f32" in d, scale=4.0, rule=rule)
    csr = csr_of(J)
    both_temperature_kinds(sg, oracle.Problem(csr=csr, h=h), lambda e: e.set_csr(*csr, h), R, 31 + rule,
                           lambda k, d: k.startswith("sweep_csr"), scale=4.0, rule=rule)


def test_dense_fp64_accumulators_at_edges(sg):
    """Integer magnitudes that need the exact paths (fp32 exact, then fp64 exact beyond 2^24), and Gaussian
    couplings in the canonical fp64 order."""
    n, R = 200, 8
    rng = np.random.RandomState(8)
    J = np.triu(rng.randint(-30000, 30001, (n, n)), 1).astype(np.float32)
    J = J + J.T
    h = rng.randint(-500, 501, n).astype(np.float32)
    both_temperature_kinds(sg, oracle.Problem(J=J, h=h), lambda e: e.set_dense(J, h), R, 41,
                           lambda k, d: "storage=f32" in d and "acc=f32" in d, scale=1e5)
    Jbig = J * 4096.0
    both_temperature_kinds(sg, oracle.Problem(J=Jbig, h=h), lambda e: e.set_dense(Jbig, h), R, 43,
                           lambda k, d: "acc=f64" in d and "ACC64=1" in k, scale=4e8)
    G = np.triu(rng.randn(n, n), 1).astype(np.float32)
    G = G + G.T
    hg = rng.randn(n).astype(np.float32)

    def canon(e):
        e.set_options(force_dense_canonical=1)
        e.set_dense(G, hg)
    both_temperature_kinds(sg, oracle.Problem(J=G, h=hg), canon, R, 45,
                           lambda k, d: "acc=f64-canonical" in d and "CANON=1" in k, scale=10.0, exact=False)


# ----------------------------------------------------------------------------- dense, cached local fields
@pytest.mark.parametrize("batched", [0, 1])
def test_dense_cached_field_forms_at_edges(sg, batched):
    n, R = 600, 8
    J = pm1(n, 6)
    h = np.random.RandomState(6).randint(-1, 2, n).astype(np.float32)
    name = "sweep_clfb_kernel" if batched else "sweep_clf_kernel"

    def setup(e):
        e.set_options(clf_batched=batched)
        e.set_field_cache("on")
        e.set_dense(J, h)

    def want(k, d):
        return k.startswith(name) and "sweep=cached-local-fields" in d and (batched or "LEAN" in k)
    both_temperature_kinds(sg, oracle.Problem(J=J, h=h), setup, R, 51 + batched, want, scale=np.sqrt(n))


def test_dense_cached_field_general_arguments_at_edges(sg):
    """The general build: sequential sites, the operator's fp32 arithmetic, recorded uniforms."""
    n, R, ns = 130, 8, 5
    J = pm1(n, 7)
    h = np.random.RandomState(7).randint(-1, 2, n).astype(np.float32)
    u = np.random.RandomState(0).rand(R, ns * n).astype(np.float32)

    def setup(e):
        e.set_field_cache("on")
        e.set_dense(J, h, storage="f32")
    for arith in (oracle.ARITH_F64, oracle.ARITH_F32):
        run_form(sg, oracle.Problem(J=J, h=h), setup, R, ns, 61, lambda k, d: k.startswith("sweep_clf_kernel") and "general" in k,
                 temps=edge_temps(R, np.sqrt(n)), site_mode=oracle.SITE_SEQUENTIAL, arith=arith, replay_u=u,
                 label=f"arith={arith}")


def test_field_cache_auto_over_a_schedule_that_reaches_zero(sg):
    """AUTO routes each replica by its acceptance, looked at every 16-sweep piece: a 40-sweep call crosses the
    piece walk while its replicas cool to exactly 0."""
    n, R = 500, 8
    J = pm1(n, 9)
    h = np.zeros(n, np.float32)

    def setup(e):
        e.set_field_cache("auto")
        e.set_dense(J, h)
    kernels = ("sweep_clf_kernel", "sweep_clfb_kernel", "sweep_dense_kernel", "mixed launch")
    run_form(sg, oracle.Problem(J=J, h=h), setup, R, 40, 71, lambda k, d: k.startswith(kernels),
             sched=cooling_sched(40, R, np.sqrt(n)))


# ----------------------------------------------------------------------------- beyond the accept table
def test_fields_beyond_the_accept_table_at_edges(sg):
    """|s_i F_i| up to several thousand: the moves beyond the 2048-entry table and those inside it both meet
    T = 0, 1e-300 and inf -- dense streaming, both cached-field forms, one-at-a-time and four-per-step CSR."""
    n, R = 260, 8
    J = int_couplings(n, 12, 120, density=0.9)
    h = np.random.RandomState(12).randint(-120, 121, n).astype(np.float32)
    prob = oracle.Problem(J=J, h=h)
    s0 = oracle.init_spins(n, R, 81)
    assert np.mean(np.abs(s0.astype(np.float32) @ J + h) > 2048) > 0.02   # a share of the moves lies beyond the table
    scale = 120.0 * np.sqrt(n * 0.9)
    both_temperature_kinds(sg, prob, lambda e: (e.set_options(sparse_route=0), e.set_dense(J, h, storage="i8")), R, 81,
                           lambda k, d: k.startswith("sweep_dense_kernel") and "storage=i8" in d, scale=scale)
    for batched in (0, 1):
        def clf(e, b=batched):
            e.set_options(clf_batched=b)
            e.set_field_cache("on")
            e.set_dense(J, h, storage="i8")
        name = "sweep_clfb_kernel" if batched else "sweep_clf_kernel"
        both_temperature_kinds(sg, prob, clf, R, 83 + batched, lambda k, d, nm=name: k.startswith(nm), scale=scale)
    csr = csr_of(J)
    assert np.diff(csr[0]).max() <= 256
    for upd in (0, 4):
        def rows(e, u=upd):
            e.set_options(csr_updates_per_step=u)
            e.set_csr(*csr, h)
        both_temperature_kinds(sg, oracle.Problem(csr=csr, h=h), rows, R, 87 + upd,
                               lambda k, d, u=upd: ("sweep_csr_rows_kernel" in k) == (u == 4) and k.startswith("sweep_csr"),
                               scale=scale)


# ----------------------------------------------------------------------------- CSR
@pytest.mark.parametrize("bits", [False, True])
@pytest.mark.parametrize("upd", [0, 2, 4, 8])
@pytest.mark.parametrize("half_h", [False, True])
def test_csr_forms_at_edges(sg, upd, bits, half_h):
    n, R = 400, 8
    J = sparse_int(n, 12, 1, 100 + n)
    h = (np.random.RandomState(13).randint(-2, 3, n) / (2.0 if half_h else 1.0)).astype(np.float32)
    csr = csr_of(J)

    def setup(e):
        e.set_options(csr_updates_per_step=upd, force_csr_bits=int(bits))
        e.set_csr(*csr, h)

    def want(k, d):
        rows = upd >= 4
        return (("sweep_csr_rows_kernel" in k) == rows and (not rows or f"<{upd} rows" in k)
                and k.startswith("sweep_csr") and ("bit spins" in k) == bits)
    both_temperature_kinds(sg, oracle.Problem(csr=csr, h=h), setup, R, 91 + upd, want, scale=4.0)


@pytest.mark.parametrize("upd", [0, 4])
def test_csr_real_valued_couplings_at_edges(sg, upd):
    n, R = 300, 8
    rng = np.random.RandomState(14)
    J = np.triu((rng.rand(n, n) < 0.04) * rng.randn(n, n), 1).astype(np.float32)
    J = J + J.T
    h = rng.randn(n).astype(np.float32)
    csr = csr_of(J)

    def setup(e):
        e.set_options(csr_updates_per_step=upd, force_csr_acc=3)
        e.set_csr(*csr, h)

    def want(k, d):
        return ("fp64 canonical sums" in k) if upd else k.startswith("sweep_csr_kernel<acc=3")
    both_temperature_kinds(sg, oracle.Problem(csr=csr, h=h), setup, R, 101 + upd, want, scale=4.0, exact=False)


def test_csr_wide_rows_at_edges(sg):
    n, R = 900, 8
    rng = np.random.RandomState(17)
    J = (np.triu(rng.rand(n, n) < 0.35, 1) * (rng.randint(0, 2, (n, n)) * 2 - 1)).astype(np.float32)
    J = J + J.T
    h = rng.randint(-2, 3, n).astype(np.float32)
    csr = csr_of(J)

    def setup(e):
        e.set_tuning(waves_per_replica=2)
        e.set_csr(*csr, h)
    both_temperature_kinds(sg, oracle.Problem(csr=csr, h=h), setup, R, 111,
                           lambda k, d: "one replica per workgroup" in k and "waves_per_replica=2" in d, scale=18.0)


def test_csr_cached_fields_at_edges(sg):
    n, R = 1000, 8
    J = sparse_int(n, 10, 2, 7)
    h = np.random.RandomState(15).randint(-3, 4, n).astype(np.float32)
    csr = csr_of(J)

    def setup(e):
        e.set_field_cache("on")
        e.set_csr(*csr, h)
    both_temperature_kinds(sg, oracle.Problem(csr=csr, h=h), setup, R, 121,
                           lambda k, d: k.startswith("sweep_clf_csr_kernel"), scale=6.0)


# ----------------------------------------------------------------------------- TSP, batches, Wolff
@pytest.mark.parametrize("par", [0, 2, 4, 8])
def test_tsp_forms_at_edges(sg, par):
    from spin_glass_anneal_rl_amd import encoders as enc
    nc, R = 17, 8
    xy = np.random.RandomState(300 + nc).rand(nc, 2) * 100.0
    dist = np.rint(np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1]) / 4.0) * 4.0
    d32, A, B, h, _ = enc.tsp_structure(dist, 200.0, 120.0, auto_scale=False)
    csr = oracle.tsp_to_csr(d32, A, B)
    prob = oracle.Problem(csr=(csr[0].astype(np.int32), csr[1], csr[2]), h=h)

    def setup(e):
        e.set_options(tsp_updates_per_step=par)
        e.set_tsp(d32, A, B, h)

    def want(k, d):
        return ("sweep_tsp_par_kernel" in k and f"x {par} updates" in k) if par else k.startswith("sweep_tsp_kernel")
    both_temperature_kinds(sg, prob, setup, R, 131 + par, want, scale=100.0, ns=4, ns_sched=18)


def test_ragged_csr_batch_at_edges(sg):
    specs = [(3, 1.0, False), (37, 0.3, True), (257, 0.05, False), (1201, 0.007, True)]
    probs = []
    for m, (n, dens, half) in enumerate(specs):
        rng = np.random.RandomState(10 + m)
        J = (np.triu(rng.rand(n, n) < dens, 1) * (rng.randint(0, 2, (n, n)) * 2 - 1)).astype(np.float32)
        J = J + J.T
        h = rng.randint(-2, 3, n).astype(np.float32) / (2.0 if half else 1.0)
        probs.append((*csr_of(J), h.astype(np.float32)))
    M, k, ns, seed = len(probs), 8, 6, 141
    R = M * k
    for sched in (None, cooling_sched(20, k, 4.0)):
        nsw = ns if sched is None else 20
        temps = np.tile(edge_temps(k, 4.0), M)
        full_sched = None if sched is None else np.ascontiguousarray(np.tile(sched, (1, M)))
        with sg.AnnealEngine(0) as e:
            e.set_csr_batch(probs)
            e.init_replicas(R, seed=seed)
            e.set_temperatures(temps)
            out = e.sweep(nsw, sched=full_sched, energy_trace=True)
            assert "ragged" in e.last_kernel(), e.last_kernel()
            spins = [e.spins(r) for r in range(R)]
            acc, att = e.stats()
        for m, p in enumerate(probs):
            prob = oracle.Problem(csr=p[:3], h=p[3])
            s = oracle.init_spins(prob.n, k, seed, replica0=m * k)
            e0 = np.asarray([oracle.energy(prob, s[r]) for r in range(k)])
            ref = oracle.sweeps(prob, s, temps[m * k:(m + 1) * k] if sched is None else sched, nsw, seed=seed,
                                replica0=m * k)
            sl = slice(m * k, (m + 1) * k)
            assert np.array_equal(out["energy_trace"][:, sl], ref["energy_trace"]), m
            assert all(np.array_equal(spins[m * k + r], s[r]) for r in range(k)), m
            assert np.array_equal(acc[sl], ref["n_accepted"]), m
            if sched is None:
                check_properties(ref, e0, temps[sl], 0, (acc[sl], att[sl]), m)


def test_dense_model_batch_at_edges(sg):
    n, M, k, ns, seed = 64, 3, 8, 6, 151
    Js = np.stack([pm1(n, 200 + m) for m in range(M)])
    hs = np.stack([np.random.RandomState(m).randint(-1, 2, n).astype(np.float32) for m in range(M)])
    R = M * k
    temps = np.tile(edge_temps(k, 8.0), M)
    with sg.AnnealEngine(0) as e:
        e.set_dense_batch(Js, hs)
        e.init_replicas(R, seed=seed)
        e.set_temperatures(temps)
        out = e.sweep(ns, energy_trace=True)
        assert f"models={M}" in e.describe(), e.describe()
        spins, (acc, att) = e.spins(), e.stats()
    for m in range(M):
        prob = oracle.Problem(J=Js[m], h=hs[m])
        sl = slice(m * k, (m + 1) * k)
        s = oracle.init_spins(n, k, seed, replica0=m * k)
        e0 = np.asarray([oracle.energy(prob, s[r]) for r in range(k)])
        ref = oracle.sweeps(prob, s, temps[sl], ns, seed=seed, replica0=m * k)
        assert np.array_equal(out["energy_trace"][:, sl], ref["energy_trace"]), m
        assert np.array_equal(spins[sl], s) and np.array_equal(acc[sl], ref["n_accepted"]), m
        check_properties(ref, e0, temps[sl], 0, (acc[sl], att[sl]), m)


@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_wolff_at_zero_and_infinite_temperature(sg, kind):
    n, R, ns, seed = 300, 8, 2, 161
    J = int_couplings(n, 16, 2, density=0.05)
    h = np.random.RandomState(16).randint(-1, 2, n).astype(np.float32)
    temps = np.asarray([0.0, INF, 0.0, INF, 1e-300, 1e30, 1.0, 5e-324])
    csr = csr_of(J)
    prob = oracle.Problem(J=J, h=h) if kind == "dense" else oracle.Problem(csr=csr, h=h)
    setup = (lambda e: (e.set_options(sparse_route=0), e.set_dense(J, h))) if kind == "dense" else (lambda e: e.set_csr(*csr, h))
    # (one kernel serves the Wolff rule, over either storage)
    run_form(sg, prob, setup, R, ns, seed, lambda k, d: d.startswith(kind), temps=temps, rule=oracle.RULE_WOLFF, recompute=True,
             label=kind)


# ----------------------------------------------------------------------------- T = 0 equals T = 1e-10
ZERO_FORMS = {
    "dense-f32": lambda J, h, csr: (lambda e: (e.set_options(sparse_route=0), e.set_dense(J, h, storage="f32"))),
    "clf": lambda J, h, csr: (lambda e: (e.set_options(clf_batched=0), e.set_field_cache("on"), e.set_dense(J, h))),
    "clfb": lambda J, h, csr: (lambda e: (e.set_options(clf_batched=1), e.set_field_cache("on"), e.set_dense(J, h))),
    "csr-1": lambda J, h, csr: (lambda e: (e.set_options(csr_updates_per_step=0), e.set_csr(*csr, h))),
    "csr-rows": lambda J, h, csr: (lambda e: (e.set_options(csr_updates_per_step=4), e.set_csr(*csr, h))),
    "csr-clf": lambda J, h, csr: (lambda e: (e.set_field_cache("on"), e.set_csr(*csr, h))),
}


@pytest.mark.parametrize("form", list(ZERO_FORMS))
def test_zero_temperature_chain_equals_tiny_temperature_chain(sg, form):
    """On integer problems every uphill move is at least 1: exp(-1 / 1e-10) is 0 in fp32, so T = 0, 5e-324 and
    1e-300 must walk the T = 1e-10 chain bit for bit -- on the GPU and in the oracle."""
    n, R, ns, seed = 400, 8, 8, 171
    J = sparse_int(n, 30, 2, 19)
    h = np.random.RandomState(19).randint(-2, 3, n).astype(np.float32)
    csr = csr_of(J)
    cold = np.asarray([0.0, 5e-324, 1e-300, 0.0, 2.0, 0.0, INF, 0.0])
    tiny = np.where(cold < 1e-10, 1e-10, cold)
    prob = oracle.Problem(csr=csr, h=h)
    runs = {}
    for name, temps in (("cold", cold), ("tiny", tiny)):
        s = oracle.init_spins(n, R, seed)
        ref = oracle.sweeps(prob, s, temps, ns, seed=seed, n_threads=8)
        with sg.AnnealEngine(0) as e:
            ZERO_FORMS[form](J, h, csr)(e)
            e.init_replicas(R, seed=seed)
            e.set_temperatures(temps)
            out = e.sweep(ns, energy_trace=True)
            runs[name] = (out["energy_trace"], e.spins(), e.stats()[0], e.last_kernel())
        runs["oracle-" + name] = (ref["energy_trace"], s, ref["n_accepted"])
    for a, b in (("cold", "tiny"), ("oracle-cold", "oracle-tiny"), ("cold", "oracle-cold")):
        for x, y in zip(runs[a][:3], runs[b][:3]):
            assert np.array_equal(x, y), (form, a, b, runs["cold"][3])


# ----------------------------------------------------------------------------- exchange
LADDERS = {
    "one-zero": [5.0, 3.0, 1.0, 0.5, 0.2, 0.1, 0.05, 0.0],
    "two-zero": [5.0, 3.0, 1.0, 0.5, 0.2, 0.1, 0.0, 0.0],
    "inf-and-zeros": [INF, 3.0, 1.0, 0.5, 5e-324, 0.0, 0.0, 1e-300],
}


def exchange_engine(sg, J, R, seed, ladder, n_ladders, R_local=None, replica0=0):
    e = sg.AnnealEngine(0)
    e.set_dense(J, np.zeros(J.shape[0], np.float32))
    e.init_replicas(R if R_local is None else R_local, seed=seed, R_global=R, replica0=replica0)
    e.set_ladder(ladder, n_ladders)
    return e


def oracle_round(temps, energies, slot, L, n_ladders, seed, rnd, att, acc, ladders=None):
    k = 0
    for l in (range(n_ladders) if ladders is None else ladders):
        sl = slice(l * L, (l + 1) * L)
        k += oracle.pt_exchange_round(temps[sl], energies, slot[sl], seed=seed, round_=rnd, ladder=l,
                                      attempts=att[sl], accepts=acc[sl])
    return k


@pytest.mark.parametrize("ladder", list(LADDERS))
@pytest.mark.parametrize("n_ladders", [1, 3])
def test_exchange_rounds_at_edge_slots(sg, ladder, n_ladders):
    """Equal energies make every attempted swap certain (min(1, exp(NaN)) is 1 in the reference's arithmetic, and
    the limit of any ladder); slot maps and counters follow the oracle round for round."""
    n, seed, L = 48, 181, 8
    R = L * n_ladders
    J = pm1(n, 21)
    temps = np.tile(np.asarray(LADDERS[ladder]), n_ladders)
    base = oracle.init_spins(n, 2, 5)
    e = exchange_engine(sg, J, R, seed, temps, n_ladders)
    try:
        for r in range(R):
            e.set_spins(r, base[0])
        slot = np.arange(R, dtype=np.int32)
        att, acc = np.zeros(R, np.int64), np.zeros(R, np.int64)
        for rnd in range(6):
            if rnd == 3:  # from here on two energies in every ladder
                for r in range(0, R, 3):
                    e.set_spins(r, base[1])
            en = e.energies()
            before = (att.sum(), acc.sum())
            want = oracle_round(temps, en, slot, L, n_ladders, seed, rnd, att, acc)
            got = e.exchange()
            assert got == want, (rnd, got, want)
            if rnd < 3:
                assert want == att.sum() - before[0] > 0, ("equal energies: every attempt swaps", rnd)
            assert np.array_equal(e.slot_map(), slot), rnd
            rep_T = np.empty(R)
            rep_T[slot] = temps
            assert np.array_equal(e.temperatures(), rep_T), rnd
        a2, c2 = e.exchange_stats()
        assert np.array_equal(a2, att) and np.array_equal(c2, acc)
    finally:
        e.close()


def test_ladder_local_exchange_at_edge_slots(sg):
    """Two engines, one ladder each, deciding their own ladder from their own energies."""
    n, seed, L, n_ladders = 48, 191, 8, 2
    R = L * n_ladders
    J = pm1(n, 22)
    temps = np.concatenate([LADDERS["two-zero"], LADDERS["inf-and-zeros"]])
    base = oracle.init_spins(n, 1, 6)[0]
    shards = [exchange_engine(sg, J, R, seed, temps, n_ladders, R_local=L, replica0=l * L) for l in range(n_ladders)]
    try:
        for e in shards:
            for r in range(L):
                e.set_spins(r, base)
        slot = np.arange(R, dtype=np.int32)
        att, acc = np.zeros(R, np.int64), np.zeros(R, np.int64)
        for rnd in range(4):
            for l, e in enumerate(shards):
                en = np.zeros(R)
                en[l * L:(l + 1) * L] = e.energies()
                before = att.sum()
                want = oracle_round(temps, en, slot, L, n_ladders, seed, rnd, att, acc, ladders=[l])
                assert e.exchange() == want == att.sum() - before > 0, (rnd, l)
                assert np.array_equal(e.slot_map()[l * L:(l + 1) * L], slot[l * L:(l + 1) * L])
        for l, e in enumerate(shards):
            a2, c2 = e.exchange_stats()
            sl = slice(l * L, (l + 1) * L)
            assert np.array_equal(a2[sl], att[sl]) and np.array_equal(c2[sl], acc[sl])
    finally:
        for e in shards:
            e.close()


def test_exchange_pairs_at_edge_slots(sg):
    n, seed, R = 48, 201, 8
    J = pm1(n, 23)
    temps = np.asarray(LADDERS["inf-and-zeros"])
    pairs = [(5, 6), (0, 1), (4, 5), (0, 6), (2, 7), (1, 3), (6, 7)]
    base = oracle.init_spins(n, 2, 7)
    e = exchange_engine(sg, J, R, seed, temps, 1)
    try:
        for r in range(R):
            e.set_spins(r, base[0])
        slot = np.arange(R, dtype=np.int32)
        att, acc = np.zeros(R, np.int64), np.zeros(R, np.int64)
        rng = np.random.RandomState(1)
        for rnd in range(4):
            if rnd == 2:
                e.set_spins(1, base[1])
                e.set_spins(6, base[1])
            en = e.energies()
            u = rng.rand(len(pairs)) if rnd % 2 else None
            want = oracle.pt_exchange_pairs(temps, en, slot, pairs, u=u, seed=seed, round_=rnd,
                                            attempts=att, accepts=acc)
            assert e.exchange_pairs(pairs, u=u) == want, rnd
            if rnd < 2:
                assert want == len(pairs), ("equal energies: every pair swaps", rnd)
            assert np.array_equal(e.slot_map(), slot), rnd
        a2, c2 = e.exchange_stats()
        assert np.array_equal(a2, att) and np.array_equal(c2, acc)
    finally:
        e.close()


def test_operator_exchange_keeps_no_swap_on_nan(sg):
    """The operator form (annealing/cuda_kernels.py:434-437) compares rand < exp(db * de): NaN never swaps, as
    in the reference."""
    n = 32
    mgr = sg.CUDAKernelManager(torch.device("cuda"))
    temps = np.asarray([1.0, 0.0, 0.0, 2.0, INF, 0.5], np.float32)
    R = len(temps)
    base = oracle.init_spins(n, 2, 8)
    spins = np.stack([base[0] if r != 4 else base[1] for r in range(R)]).astype(np.int8)
    energies = np.asarray([-10.0, -10.0, -10.0, -10.0, -4.0, -10.0], np.float32)
    for u in (np.zeros(R - 1, np.float32), np.random.RandomState(2).rand(R - 1).astype(np.float32)):
        s_ref, e_ref = spins.copy(), energies.copy()
        want = oracle.pt_exchange_operator(s_ref, e_ref, temps, u)
        sp = torch.from_numpy(spins.astype(np.float32)).cuda()
        en = torch.from_numpy(energies.copy()).cuda()
        got = mgr.parallel_tempering_exchange_optimized(sp, en, torch.from_numpy(temps).cuda(), _uniforms=u)
        assert got == want
        assert np.array_equal(sp.cpu().numpy().astype(np.int8), s_ref)
        assert np.array_equal(en.cpu().numpy(), e_ref)
    # pairs (1.0, 0.0), (0.0, 0.0), (0.0, 2.0) have NaN arguments: not swapped even at u = 0
    s0, e0 = spins.copy(), energies.copy()
    oracle.pt_exchange_operator(s0, e0, temps, np.zeros(R - 1, np.float32))
    assert np.array_equal(e0[:3], energies[:3]) and np.array_equal(s0[:3], spins[:3])


def test_scheduler_with_infinite_beta_equals_huge_beta(sg):
    """SpinGlassScheduler.anneal on a dense +-1 problem (field_cache="auto"): a ladder ending at beta = inf (T = 0)
    and the same ladder ending at beta = 1e10 give one result -- the cold end quenches greedily either way and
    exchanges at equal energies swap either way.  (Odd n: the local fields of the +-1 couplings are even and
    can be 0, so a quenched replica still meets flat moves.)"""
    n = 401
    m = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=False))
    m.set_couplings_from_matrix(torch.from_numpy(pm1(n, 24)))
    runs = []
    for last in (INF, 1e10):
        betas = np.concatenate([np.geomspace(0.05, 3.0, 15), [last]])
        runs.append(sg.SpinGlassScheduler(device="cuda", random_seed=13).anneal(
            m, n_replicas=16, n_sweeps=300, beta_schedule=betas, exchange_interval=10))
    assert runs[0].best_energy == runs[1].best_energy
    assert torch.equal(runs[0].best_configuration, runs[1].best_configuration)
    assert runs[0].energy_history == runs[1].energy_history


# ----------------------------------------------------------------------------- refusals
def test_negative_and_nan_temperatures_are_refused(sg):
    n, R, seed = 96, 8, 211
    J = pm1(n, 25)
    h = np.zeros(n, np.float32)
    temps = edge_temps(R, 4.0)
    prob = oracle.Problem(J=J, h=h)
    with sg.AnnealEngine(0) as e:
        e.set_dense(J, h)
        e.init_replicas(R, seed=seed)
        e.set_ladder(temps)
        e.sweep(2)
        state = (e.temperatures(), e.slot_map(), e.spins(), e.energies(), e.counters())
        for bad in (-1.0, -0.0, -INF, float("nan")):
            t = temps.copy()
            t[3] = bad
            with pytest.raises(sg.AnnealingError, match="sga_set_temperatures"):
                e.set_temperatures(t)
            with pytest.raises(sg.AnnealingError, match="sga_set_ladder"):
                e.set_ladder(t)
            sched = np.tile(temps, (20, 1))
            sched[17, 5] = bad                  # in the second 16-sweep piece: refused before the first runs
            with pytest.raises(sg.AnnealingError, match="sga_sweep"):
                e.sweep(20, sched=sched)
            with pytest.raises(sg.AnnealingError, match="sga_sweep"):
                e.sweep(3, sched=np.full(3, bad))
            now = (e.temperatures(), e.slot_map(), e.spins(), e.energies(), e.counters())
            assert all(np.array_equal(a, b) for a, b in zip(state, now)), bad
        assert e.n_ladders == 1
        s = oracle.init_spins(n, R, seed)
        ref = oracle.sweeps(prob, s, temps, 2, seed=seed)
        ref = oracle.sweeps(prob, s, temps, 3, seed=seed, sweep0=2, energy=ref["energy"],
                            best_energy=ref["best_energy"])
        out = e.sweep(3, energy_trace=True)
        assert np.array_equal(out["energy_trace"], ref["energy_trace"]) and np.array_equal(e.spins(), s)
