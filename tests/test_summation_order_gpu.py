"""The canonical fp64 summation order on the GPU, on problems where the order shows (tests/canonical_sum.py).

tests/test_summation_order_host.py proves on the CPU, for every run used here, that the oracle follows the stated order
and that a kernel summing in another order (left to right, lane products k-major, another tree, super-chunks grouped
by wave, 4 virtual waves, lanes folded per pass) changes at least a quarter of the proposed fp32 row sums -- and, for
the production runs without per-update records, at least one accept decision.  Here every sweep form of the
f64-canonical class walks those runs: accept and dE records, final spins, acceptance counters, tracked energies and
best states bit for bit, each case asserting which form ran.  Single-site operators and from-scratch energies are
compared with canonical_sum directly.  No tolerance anywhere.
"""
import numpy as np
import pytest

import canonical_sum as cs
import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


_refs = {}


def reference(cfg, e0):
    """The oracle's run from the engine's initial energies (cached: many forms walk one run)."""
    key = (cfg["name"], e0.tobytes())
    if key not in _refs:
        _refs[key] = cs.oracle_run(cfg, energy=e0)
    return _refs[key]


def set_problem(e, prob, wide_extents=False):
    if prob.J is not None:
        e.set_dense(prob.J, prob.h)
    else:
        rp = prob.csr[0].astype(np.int64) if wide_extents else prob.csr[0]
        e.set_csr(rp, prob.csr[1], prob.csr[2], prob.h)


def run_case(sg, name, want, options=None, waves=0, wide_extents=False):
    """One forced form on one run of canonical_sum.RUNS against the oracle, everything on bits."""
    cfg = cs.run_setup(name)
    prob, R, ns = cfg["prob"], cfg["R"], cfg["ns"]
    traced = cfg["kind"] != "production"
    with sg.AnnealEngine(0) as e:
        e.set_options(options or {})
        if waves:
            e.set_tuning(waves_per_replica=waves)
        set_problem(e, prob, wide_extents)
        e.set_update_rule(cfg["rule"])
        e.init_replicas(R, seed=cfg["seed"], s0=cfg["s0"])
        e.set_temperatures(cfg["temps"])
        e0 = e.energies()
        out = e.sweep(ns, site_mode=cfg["mode"], replay_site=cfg["site"], replay_u=cfg["u"], energy_trace=True,
                      trace=traced)
        k, d = e.last_kernel(), e.describe()
        spins, energy, stats = e.spins(), e.energies(), e.stats()
        best = [e.best(r) for r in range(R)]
    tag = (name, k, d)
    assert "acc=f64-canonical" in d and want(k, d), tag
    ref = reference(cfg, e0)
    if traced:
        assert np.array_equal(out["accept_trace"], ref["accept_trace"]), tag
        bad = np.nonzero(out["dE_trace"] != ref["dE_trace"])
        assert bad[0].size == 0, (tag, "dE records", bad[0].size, out["dE_trace"][bad][:4], ref["dE_trace"][bad][:4])
    assert np.array_equal(spins, ref["spins"]), tag
    assert np.array_equal(stats[0], ref["n_accepted"]), tag
    assert np.array_equal(out["energy_trace"], ref["energy_trace"]), tag
    assert np.array_equal(energy, ref["energy"]), tag
    for r in range(R):
        assert best[r][0] == ref["best_energy"][r] and np.array_equal(best[r][1], ref["best_spins"][r]), (tag, r)
    assert np.array_equal(spins[:, prob.ballast], np.tile(prob.ballast_spin[prob.ballast], (R, 1))), (tag, "ballast flipped")
    assert ref["n_accepted"].min() > 0, tag


# ----------------------------------------------------------------------------- dense
# (problem, requested waves) -> (waves, chunks per wave, streaming) the canonical geometry gives: a wave owns whole
# super-chunks, so there are never more waves than super-chunks
DENSE_GEOMETRIES = [
    ("d700", 1, 1, 4, False), ("d700", 5, 1, 4, False),
    ("d2501", 1, 1, 12, True), ("d2501", 2, 2, 8, False), ("d2501", 3, 3, 4, False), ("d2501", 16, 3, 4, False),
    ("d5000", 1, 1, 20, True), ("d5000", 2, 2, 12, True), ("d5000", 3, 3, 8, False), ("d5000", 5, 5, 4, False),
    ("d6002", 1, 1, 24, True), ("d6002", 2, 2, 12, True), ("d6002", 3, 3, 8, False), ("d6002", 5, 5, 8, False),
    ("d6002", 8, 6, 4, False), ("d6002", 16, 6, 4, False),
]


def want_dense(w, cpw, streaming, lean):
    def want(k, d):
        return (k.startswith("sweep_dense_kernel<float") and "ACC64=1" in k and "CANON=1" in k and f"LEAN={int(lean)}" in k
                and f"waves_per_replica={w} " in d and f"chunks_per_wave={cpw}{'(streaming)' if streaming else ''} " in d)
    return want


@pytest.mark.parametrize("kind", ["philox", "production"])
@pytest.mark.parametrize("key,ask,w,cpw,streaming", DENSE_GEOMETRIES)
def test_dense_geometries_follow_the_canonical_order(sg, key, ask, w, cpw, streaming, kind):
    run_case(sg, f"{key}-{kind}", want_dense(w, cpw, streaming, kind == "production"), waves=ask)


@pytest.mark.parametrize("name,ask,w,cpw,streaming", [
    ("d700-replay", 0, 1, 4, False), ("d700-glauber", 1, 1, 4, False), ("d700-heat-bath", 1, 1, 4, False),
    ("d700-sequential", 1, 1, 4, False), ("d2501-replay", 1, 1, 12, True), ("d2501-replay", 3, 3, 4, False)])
@pytest.mark.parametrize("look", [1, 0])
def test_dense_rules_site_orders_and_look_ahead(sg, name, ask, w, cpw, streaming, look):
    run_case(sg, name, want_dense(w, cpw, streaming, False), options={"look_ahead": look}, waves=ask)


def test_dense_general_build_under_production_arguments(sg):
    run_case(sg, "d2501-production", want_dense(2, 8, False, False), options={"force_general": 1}, waves=2)


# ----------------------------------------------------------------------------- CSR
def want_rows(upd, bits):
    return lambda k, d: ("sweep_csr_rows_kernel" in k and f"<{upd} rows" in k and "fp64 canonical sums" in k
                         and (("bit spins" in k) == bits) and f"updates_per_step={upd}" in d)


def want_narrow(bits):
    return lambda k, d: (k.startswith("sweep_csr_kernel<acc=3") and (("bit spins" in k) == bits)
                         and "waves_per_replica=1 " in d and "updates_per_step" not in d)


def want_wide(w, bits):
    return lambda k, d: (k.startswith("sweep_csr_kernel<acc=3, one replica per workgroup") and f"x {w} wave(s)" in k
                         and (("bit spins" in k) == bits) and f"waves_per_replica={w} " in d
                         and (("spins=lds-bits" in d) == bits))


@pytest.mark.parametrize("bits", [False, True])
@pytest.mark.parametrize("upd", [8, 4])
@pytest.mark.parametrize("name", ["c8-production", "c64-production", "c64-sorted-production"])
def test_csr_several_updates_per_step_follow_the_canonical_order(sg, name, upd, bits):
    """The rows kernel serves production sweeps (a traced sweep of the same engine takes the narrow general build:
    the narrow cases below), so the order shows through decisions only -- the host file proves that it does."""
    run_case(sg, name, want_rows(upd, bits), options={"csr_updates_per_step": upd, "force_csr_bits": int(bits)})


@pytest.mark.parametrize("name", ["c8-philox", "c64-philox", "c64-replay", "c64-sorted-philox", "c64-production",
                                  "c300-philox", "c300-production", "c1200-philox"])
@pytest.mark.parametrize("bits", [False, True])
def test_csr_narrow_form_follows_the_canonical_order(sg, name, bits):
    """One update at a time, one replica per wave: a lane adds several entries of a long row.  (The pair look-ahead,
    "csr_updates_per_step" = 1 | 2, exists for accept-table problems only -- sweep_csr_impl.h takes it under LEAN and
    TABLE -- so the f64-canonical class never runs it and there is no pair form to pin.)"""
    run_case(sg, name, want_narrow(bits), options={"csr_updates_per_step": 0, "force_csr_bits": int(bits)}, waves=1)


@pytest.mark.parametrize("name", ["c300-philox", "c300-production", "c1200-philox"])
def test_csr_narrow_form_on_rows_without_slots(sg, name):
    """"csr_slots" = 0 and one wave per replica: the layout stays unslotted (the wide forms would pad it on demand)."""
    def want(k, d):
        return want_narrow(False)(k, d) and "rows=64-entry-slots" not in d
    run_case(sg, name, want, options={"csr_updates_per_step": 0, "csr_slots": 0}, waves=1)


@pytest.mark.parametrize("kind", ["philox", "production"])
@pytest.mark.parametrize("bits", [False, True])
@pytest.mark.parametrize("key,ask,w", [("c300", 2, 2), ("c300", 3, 4), ("c300", 8, 8), ("c1200", 2, 2), ("c1200", 3, 4),
                                       ("c1200", 4, 4), ("c1200", 8, 8)])
def test_csr_wide_rows_follow_the_canonical_order(sg, key, ask, w, bits, kind):
    run_case(sg, f"{key}-{kind}", want_wide(w, bits), options={"force_csr_bits": int(bits)}, waves=ask)


@pytest.mark.parametrize("options,wide_extents", [({"zero_slot_every": 3}, False),
                                                  ({"zero_slot_every": 1, "force_csr_bits": 1}, False), ({}, True),
                                                  ({"force_csr_bits": 1}, True)])
@pytest.mark.parametrize("key,w", [("c300", 4), ("c1200", 2), ("c1200", 8)])
def test_csr_wide_row_layouts_follow_the_canonical_order(sg, key, w, options, wide_extents):
    """All-zero slots inside the layout, 64-bit extents (sga_set_csr64)."""
    bits = bool(options.get("force_csr_bits"))
    run_case(sg, f"{key}-philox", want_wide(w, bits), options=options, waves=w, wide_extents=wide_extents)


# ----------------------------------------------------------------------------- many models
def test_ragged_csr_batch_beside_an_integer_model(sg):
    """One probe / ballast model makes the whole batch canonical: every model walks its one-model oracle run."""
    rng = np.random.RandomState(41)
    n_int = 90
    Ji = (np.triu(rng.rand(n_int, n_int) < 0.1, 1) * (rng.randint(0, 2, (n_int, n_int)) * 2 - 1)).astype(np.float32)
    Ji = Ji + Ji.T
    models = [cs.problem("c64", True), cs.Problem("integer", n_int, rng.randint(-2, 3, n_int).astype(np.float32),
                                                   np.arange(n_int), np.zeros(n_int, np.int8), csr=cs.to_csr(Ji)),
              cs.problem("c300", True)]
    M, k, ns, seed = len(models), 3, 3, 4141
    n_max = max(p.n for p in models)
    s0 = np.zeros((M * k, n_max), np.int8)
    temps = np.zeros(M * k)
    for m, p in enumerate(models):
        s0[m * k:(m + 1) * k, :p.n] = p.s0(k, seed, replica0=m * k)
        temps[m * k:(m + 1) * k] = p.probe_scale() * np.asarray([2.0, 1.0, 0.5])
    with sg.AnnealEngine(0) as e:
        e.set_csr_batch([(*p.csr, p.h) for p in models])
        e.init_replicas(M * k, seed=seed, s0=s0)
        e.set_temperatures(temps)
        e0 = e.energies()
        out = e.sweep(ns, energy_trace=True, trace=True)
        kname, d = e.last_kernel(), e.describe()
        spins = [e.spins(r) for r in range(M * k)]
        acc = e.stats()[0]
    assert "ragged" in kname and "acc=f64-canonical" in d and f"models={M}" in d, (kname, d)
    for m, p in enumerate(models):
        sl = slice(m * k, (m + 1) * k)
        s = s0[sl, :p.n].copy()
        ref = oracle.sweeps(p.oracle_problem(), s, temps[sl], ns, seed=seed, replica0=m * k, energy=e0[sl], trace=True)
        for r in range(k):
            rows = out["accept_trace"][m * k + r].reshape(ns, n_max)[:, :p.n].reshape(-1)
            assert np.array_equal(rows, ref["accept_trace"][r]), (m, r)
            rows = out["dE_trace"][m * k + r].reshape(ns, n_max)[:, :p.n].reshape(-1)
            assert np.array_equal(rows, ref["dE_trace"][r]), (m, r)
            assert np.array_equal(spins[m * k + r], s[r]), (m, r)
            assert np.array_equal(s[r][p.ballast], p.ballast_spin[p.ballast]), (m, r, "a ballast spin flipped")
        assert np.array_equal(out["energy_trace"][:, sl], ref["energy_trace"]), m
        assert np.array_equal(acc[sl], ref["n_accepted"]), m


def test_dense_batch_of_canonical_models(sg):
    models = [cs.dense_problem(700, 51, True), cs.dense_problem(700, 52, True)]
    M, k, ns, seed, n = 2, 3, 2, 5151, 700
    s0 = np.concatenate([p.s0(k, seed, replica0=m * k) for m, p in enumerate(models)])
    temps = np.tile(models[0].probe_scale() * np.asarray([2.0, 1.0, 0.5]), M)
    with sg.AnnealEngine(0) as e:
        e.set_dense_batch(np.stack([p.J for p in models]), np.stack([p.h for p in models]))
        e.init_replicas(M * k, seed=seed, s0=s0)
        e.set_temperatures(temps)
        e0 = e.energies()
        out = e.sweep(ns, energy_trace=True, trace=True)
        kname, d = e.last_kernel(), e.describe()
        spins, acc = e.spins(), e.stats()[0]
    assert "acc=f64-canonical" in d and f"models={M}" in d and kname.startswith("sweep_dense_kernel"), (kname, d)
    for m, p in enumerate(models):
        sl = slice(m * k, (m + 1) * k)
        s = s0[sl].copy()
        ref = oracle.sweeps(p.oracle_problem(), s, temps[sl], ns, seed=seed, replica0=m * k, energy=e0[sl], trace=True)
        assert np.array_equal(out["accept_trace"][sl], ref["accept_trace"]), m
        assert np.array_equal(out["dE_trace"][sl], ref["dE_trace"]), m
        assert np.array_equal(spins[sl], s) and np.array_equal(acc[sl], ref["n_accepted"]), m
        assert np.array_equal(s[:, p.ballast], np.tile(p.ballast_spin[p.ballast], (k, 1))), (m, "a ballast spin flipped")
        assert np.array_equal(out["energy_trace"][:, sl], ref["energy_trace"]), m


# ----------------------------------------------------------------------------- single-site operators
@pytest.mark.parametrize("key", ["d700", "d2501", "d5000", "c8", "c64", "c300", "c1200"])
def test_single_site_operators_against_the_reference_sums(sg, key):
    """local_fields on every probe site, flip, update (accepted and refused) against canonical_sum itself."""
    prob = cs.problem(key, False)
    s = prob.s0(2, 77)
    T = prob.probe_scale()

    def fields(sites, spins):
        return prob.row_sums(sites, np.repeat(spins[None, :], len(sites), 0)) + prob.h[sites].astype(np.float64)
    with sg.AnnealEngine(0) as e:
        set_problem(e, prob)
        e.init_replicas(2, seed=77, s0=s)
        assert "acc=f64-canonical" in e.describe()
        got = e.local_fields(1, prob.probes)
        want = fields(prob.probes, s[1])
        assert np.array_equal(got, want), (key, int(np.sum(got != want)), len(want))
        cur = s[1].copy()
        for site in prob.probes[[0, 5, len(prob.probes) // 2, -1]]:
            dE = 2.0 * float(cur[site]) * fields(np.asarray([site]), cur)[0]
            assert e.flip(1, int(site)) == dE, (key, site)
            cur[site] = -cur[site]
        n_acc = n_ref = 0
        for j, site in enumerate(prob.probes[3:43]):
            f = fields(np.asarray([site]), cur)
            u = np.float32(0.0 if j % 2 else 0.999)
            acc, rec = cs.decide(cs.METROPOLIS, cur[[site]].astype(np.float64), f, T / 8.0, np.asarray([u]))
            a, dE = e.update(1, int(site), T / 8.0, float(u))
            assert (a, dE) == (bool(acc[0]), 2.0 * float(cur[site]) * f[0]), (key, site)
            if acc[0]:
                cur[site] = -cur[site]
            n_acc, n_ref = n_acc + int(a), n_ref + int(not a)
        assert n_acc > 0 and n_ref > 0
        assert np.array_equal(e.spins(1), cur) and np.array_equal(e.spins(0), s[0])


# ----------------------------------------------------------------------------- from-scratch energies, Wolff
DISTINCT = 4  # the reference energies are walked in Python: replicas repeat four spin vectors
_quad = {}


def quad_case(kind, n):
    """(problem, spin vectors [DISTINCT, n], their reference energies), cached over the cases."""
    if (kind, n) not in _quad:
        prob = cs.quad_problem(n, 31, as_csr=(kind == "csr"))
        S = cs.quad_spins(n, DISTINCT, 900 + n)
        _quad[(kind, n)] = (prob, S, np.asarray([cs.chain_energy(prob, s) for s in S]))
    return _quad[(kind, n)]


@pytest.mark.parametrize("batched", [1, 0])
@pytest.mark.parametrize("R", [1, 5, 64, 200])
@pytest.mark.parametrize("kind,n", [("dense", 600), ("dense", 2600), ("dense", 4400), ("csr", 600)])
def test_from_scratch_energies_carry_the_canonical_bits(sg, kind, n, R, batched):
    """sga_init_replicas, sga_recompute_energies and sga_set_spins on the quad problem (every row sum order sensitive,
    none dominates X; the host file asserts that every decoy order moves E): one, three and five super-chunks per
    dense row, 599 entries per CSR row.  Two deviations these cases found are fixed in csrc/sga_misc.hip: the CSR
    energy kernels folded one virtual wave instead of eight, and energy_dense_kernel<float> carried a lane's partial
    across super-chunks with one fold per row."""
    prob, S4, want4 = quad_case(kind, n)
    idx = np.arange(R) % DISTINCT
    S, want = np.ascontiguousarray(S4[idx]), want4[idx]
    with sg.AnnealEngine(0) as e:
        e.set_options(batched_energy=batched)
        set_problem(e, prob)
        e.init_replicas(R, seed=1, s0=S)
        assert "acc=f64-canonical" in e.describe()
        assert np.array_equal(e.energies(), want), (kind, n, R, batched, "sga_init_replicas")
        e.recompute_energies()
        assert np.array_equal(e.energies(), want), (kind, n, R, batched, "sga_recompute_energies")
        r = R - 1
        e.set_spins(r, S4[3])
        assert e.energies()[r] == want4[3], (kind, n, R, batched, "sga_set_spins")


def test_ragged_batch_energies_carry_the_canonical_bits(sg):
    """energy_csr_ragged_kernel: the quad CSR problem (rows of 599 and 399 entries) beside an integer model."""
    rng = np.random.RandomState(43)
    n_int = 90
    Ji = (np.triu(rng.rand(n_int, n_int) < 0.1, 1) * (rng.randint(0, 2, (n_int, n_int)) * 2 - 1)).astype(np.float32)
    Ji = Ji + Ji.T
    hi = rng.randint(-2, 3, n_int).astype(np.float32)
    quads = [quad_case("csr", 600), quad_case("csr", 400)]
    k = DISTINCT
    n_max = 600
    s_int = oracle.init_spins(n_int, k, 7)
    s0 = np.zeros((3 * k, n_max), np.int8)
    s0[0:k, :600], s0[k:2 * k, :n_int], s0[2 * k:, :400] = quads[0][1], s_int, quads[1][1]
    want = np.concatenate([quads[0][2], oracle.energy(oracle.Problem(J=Ji, h=hi), s_int), quads[1][2]])
    with sg.AnnealEngine(0) as e:
        e.set_csr_batch([(*quads[0][0].csr, quads[0][0].h), (*cs.to_csr(Ji), hi), (*quads[1][0].csr, quads[1][0].h)])
        e.init_replicas(3 * k, seed=1, s0=s0)
        d = e.describe()
        assert "acc=f64-canonical" in d and "models=3" in d, d
        assert np.array_equal(e.energies(), want), "sga_init_replicas"
        e.recompute_energies()
        assert np.array_equal(e.energies(), want), "sga_recompute_energies"
        e.set_spins(0, quads[0][1][2])
        e.set_spins(3 * k - 1, quads[1][1][0])
        got = e.energies()
        assert got[0] == quads[0][2][2] and got[3 * k - 1] == quads[1][2][0], "sga_set_spins"


@pytest.mark.parametrize("kind,n", [("dense", 1100), ("csr", 400)])
def test_wolff_kernel_row_sums_follow_the_canonical_order(sg, kind, n):
    """The Wolff kernel forms its own row sums (sweep_wolff.hip, row_dot / full_energy) only when the per-move dE record
    is asked for: one traced sweep, dE records, spins and cluster sizes against the oracle bit for bit.  The quad
    problem keeps its cancellation under cluster moves (groups flip whole), two super-chunks per dense row, 399
    entries per CSR row.  The uniforms are Philox's: a recorded stream would need one uniform per candidate bond, up
    to n^2 / 2 per move here, because the big negative bonds always join."""
    prob = cs.quad_problem(n, 61, as_csr=(kind == "csr"))
    R, seed = 2, 616
    temps = prob.probe_scale() * np.asarray([1.0, 0.25])
    s0 = cs.quad_spins(n, R, 617)
    s = s0.copy()
    ref = oracle.sweeps(prob.oracle_problem(), s, temps, 1, rule=oracle.RULE_WOLFF, seed=seed, recompute_energy=True,
                        trace=True, n_threads=R)
    with sg.AnnealEngine(0) as e:
        set_problem(e, prob)
        e.set_update_rule(sg._native.RULE_WOLFF)
        e.init_replicas(R, seed=seed, s0=s0)
        e.set_temperatures(temps)
        assert "acc=f64-canonical" in e.describe()
        out = e.sweep(1, energy_trace=True, trace=True)
        bad = np.nonzero(out["dE_trace"] != ref["dE_trace"])
        assert bad[0].size == 0, (kind, bad[0].size, out["dE_trace"][bad][:4], ref["dE_trace"][bad][:4])
        assert np.array_equal(e.spins(), s)
        assert np.array_equal(e.stats()[0], ref["n_accepted"])
        want = [cs.chain_energy(prob, s[r]) for r in range(R)]
        assert np.array_equal(out["energy_trace"][0], want) and np.array_equal(e.energies(), want)
    m = n // 4
    assert all(np.array_equal(s[:, :m], s[:, q * m:(q + 1) * m]) for q in range(1, 4)), "a group was split"
    assert np.count_nonzero(ref["dE_trace"]) > n, "the moves must change the energy"
