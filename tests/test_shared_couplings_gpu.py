"""Shared-coupling batches (sga_set_dense_shared: ONE coupling matrix, M field vectors) through the C ABI, on the GPU.

Each model must walk the chain of a one-model engine holding (J, h_m) started at replica0 = m k, in whatever form runs:
every case compares energy traces, final spins, energies, acceptance counters, per-replica bests and their spins, swap
counts and the slot map with per-model oracle runs BIT FOR BIT (one ladder per model, an exchange after every sweep
call), asserts from last_kernel() that the intended kernel ran, and asserts from the ORACLE's counters that every model
both accepted and rejected something.  One case holds the shared engine against sga_set_dense_batch on the tiled J."""
import numpy as np
import pytest

import oracle
from batch_fx_cases import assert_same, both_branches, ladder, oracle_batch, scan_words, sym

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def pm1(n, seed):
    return sym(np.random.RandomState(seed).randint(0, 2, (n, n)) * 2 - 1)


def int_couplings(n, seed, amp):
    return sym(np.random.RandomState(seed).randint(-amp, amp + 1, (n, n)))


def int_fields(n, M, seed, amp=1):
    return np.stack([np.random.RandomState(seed + m).randint(-amp, amp + 1, n).astype(np.float32) for m in range(M)])


def tiled(J, M):
    return np.ascontiguousarray(np.broadcast_to(J, (M,) + J.shape))


def truth(J, hs, k, seed, temps, plan, **kw):
    """Per-model oracle runs: model m is the one-model problem (J, h_m) at replica0 = m k."""
    ref = oracle_batch(tiled(J, hs.shape[0]), hs, k, seed, temps, plan, **kw)
    both_branches(ref, hs.shape[0], k)
    return ref


def engine_run(sg, J, hs, k, seed, slot_temps, plan, cache="off", storage="auto", options=None, exchange=True, stacked=False,
               **sweep_kw):
    M = hs.shape[0]
    with sg.AnnealEngine(0) as e:
        e.set_options(options or {})
        e.set_field_cache(cache)
        if stacked:
            e.set_dense_batch(tiled(J, M), hs, storage=storage)
        else:
            e.set_dense_shared(J, hs, storage=storage)
        e.init_replicas(M * k, seed=seed)
        e.set_ladder(slot_temps, n_ladders=M)
        traces, kernels, swaps, acc_tr, dE_tr = [], [], [], [], []
        for ns in plan:
            out = e.sweep(ns, energy_trace=True, **sweep_kw)
            traces.append(out["energy_trace"])
            kernels.append(e.last_kernel())
            if sweep_kw.get("trace"):
                acc_tr.append(out["accept_trace"])
                dE_tr.append(out["dE_trace"])
            if exchange:
                swaps.append(e.exchange())
        bests = [e.best(r) for r in range(M * k)]
        return dict(traces=traces, spins=e.spins(), energy=e.energies().copy(), acc=e.stats()[0].copy(),
                    best_e=np.asarray([b[0] for b in bests]), best_s=np.stack([b[1] for b in bests]), swaps=swaps,
                    slot=e.slot_map().copy(), kernels=kernels, describe=e.describe(), explain=e.explain_route(),
                    accept_trace=acc_tr, dE_trace=dE_tr, scan=e.scan_summary(), checksum=e.problem_checksum())


def ran(got, name):
    return all(kname.startswith(name) for kname in got["kernels"])


# ----------------------------------------------------------------------------- 1. one row per proposal
@pytest.mark.parametrize("storage,rows", [("f32", "float"), ("i8", "int8_t")])
def test_row_per_proposal(sg, storage, rows):
    n, M, k = 96, 3, 4
    J, hs = pm1(n, 11), int_fields(n, M, 100)
    assert not np.array_equal(hs[0], hs[1]) and not np.array_equal(hs[1], hs[2])
    temps, seed, plan = np.tile(ladder(k, 3.0, 0.5), M), 0x5A4ED001, (2, 3)
    ref = truth(J, hs, k, seed, temps, plan)
    got = engine_run(sg, J, hs, k, seed, temps, plan, storage=storage)
    assert ran(got, f"sweep_dense_kernel<{rows},"), got["kernels"]
    assert f"shared-J models={M}" in got["describe"] and f"storage={storage}" in got["describe"], got["describe"]
    assert f"shared-J models={M}" in got["explain"], got["explain"]
    assert_same(got, ref)


def test_row_per_proposal_real_valued(sg):
    """A Gaussian J whose magnitudes spread over six decades (no fp64 sum of a row is exact in every order: the canonical
    summation class) under real-valued fields."""
    n, M, k = 64, 3, 4
    rng = np.random.RandomState(21)
    J = sym(rng.randn(n, n) * 10.0 ** rng.uniform(-4.0, 2.0, (n, n)))
    hs = np.stack([(np.random.RandomState(30 + m).randn(n) * 0.5).astype(np.float32) for m in range(M)])
    temps, seed, plan = np.tile(ladder(k, 3.0, 0.5), M), 0x5A4ED002, (2, 3)
    ref = truth(J, hs, k, seed, temps, plan)
    got = engine_run(sg, J, hs, k, seed, temps, plan)
    assert ran(got, "sweep_dense_kernel<float,") and "acc=f64-canonical" in got["describe"], (got["kernels"], got["describe"])
    assert_same(got, ref)


# ----------------------------------------------------------------------------- 2. bit-planes
def test_bit_planes_are_served(sg):
    n, M, k = 300, 3, 4
    J, hs = pm1(n, 12), int_fields(n, M, 200)
    temps, seed, plan = np.tile(ladder(k, 1.5 * np.sqrt(n), 0.15 * np.sqrt(n)), M), 0x5A4ED003, (2, 3)
    ref = truth(J, hs, k, seed, temps, plan)
    got = engine_run(sg, J, hs, k, seed, temps, plan, storage="t2")
    assert ran(got, "sweep_dense_kernel<Tern2,"), got["kernels"]
    assert "storage=t2" in got["describe"] and "storage=t2" in got["explain"], got["describe"]
    assert_same(got, ref)
    # the stacked batch refuses this storage: it has a row i per model
    with sg.AnnealEngine(0) as e:
        with pytest.raises(sg.AnnealingError, match="bit-plane storage needs one model"):
            e.set_dense_batch(tiled(J, M), hs, storage="t2")


# ----------------------------------------------------------------------------- 3. row-shared windows
def rs_options(W):
    return {"row_shared": 1, "row_shared_window": W}


RS_CASES = {
    # name: (n, M, k, W, J, fields, (tmax, tmin), kernel)
    "two-windows-second-partial": (300, 3, 4, 256, lambda: pm1(300, 13), lambda: int_fields(300, 3, 300), (26.0, 2.6),
                                   "sweep_dense_rs<int8_t, planes=1, W=256>"),
    "planes-beyond-one-group": (1100, 2, 3, 1024, lambda: pm1(1100, 14), lambda: int_fields(1100, 2, 400), (50.0, 5.0),
                                "sweep_dense_rs<int8_t, planes=1, W=1024>"),
    "several-magnitude-planes": (300, 3, 4, 512, lambda: int_couplings(300, 15, 5), lambda: int_fields(300, 3, 500, 2),
                                 (80.0, 8.0), "sweep_dense_rs<int8_t, planes=3, W=512>"),
    "fields-m-times-ones": (300, 3, 4, 256, lambda: pm1(300, 16),
                            lambda: np.stack([np.full(300, float(m), np.float32) for m in range(3)]), (26.0, 2.6),
                            "sweep_dense_rs<int8_t, planes=1, W=256>"),
}


@pytest.mark.parametrize("name", sorted(RS_CASES))
def test_row_shared_windows(sg, name):
    n, M, k, W, make_J, make_h, (tmax, tmin), kernel = RS_CASES[name]
    J, hs = make_J(), make_h()
    temps, seed, plan = np.tile(ladder(k, tmax, tmin), M), 0x5A4ED100 + n + W, (2, 3)
    ref = truth(J, hs, k, seed, temps, plan)
    if name == "fields-m-times-ones":  # one J, one seed per replica: what differs between the models' counters is h
        rate = [int(ref["acc"][m * k:(m + 1) * k].sum()) for m in range(M)]
        assert len(set(rate)) == M, rate
    got = engine_run(sg, J, hs, k, seed, temps, plan, options=rs_options(W))
    assert ran(got, kernel), got["kernels"]
    assert "resident bit-planes" in got["kernels"][0] or "planes=8" in kernel, got["kernels"]
    assert f"sweep=row-shared(W={W}" in got["describe"] and f"shared-J models={M}" in got["describe"], got["describe"]
    assert "sweep=row-shared" in got["explain"], got["explain"]
    assert_same(got, ref)
    # the same chain as the row-per-proposal kernel of the same engine
    rows = engine_run(sg, J, hs, k, seed, temps, plan, options={"row_shared": 0})
    assert ran(rows, "sweep_dense_kernel<"), rows["kernels"]
    assert_same(rows, ref)


def test_row_shared_windows_fp32_rows(sg):
    """fp32 rows: the chain's corrections are gathered from the fp32 matrix (planes = 3: no bit chain)."""
    n, M, k, W = 300, 3, 4, 256
    J, hs = int_couplings(n, 17, 3), int_fields(n, M, 600)
    temps, seed, plan = np.tile(ladder(k, 60.0, 6.0), M), 0x5A4ED200, (2, 3)
    ref = truth(J, hs, k, seed, temps, plan)
    got = engine_run(sg, J, hs, k, seed, temps, plan, storage="f32", options=rs_options(W))
    assert ran(got, "sweep_dense_rs<float, planes=3, W=256>"), got["kernels"]
    assert_same(got, ref)


def test_row_shared_shards_cut_inside_a_model(sg):
    n, M, k, W = 300, 3, 4, 256
    R = M * k  # the cut at 6 falls inside model 1
    J, hs = pm1(n, 18), int_fields(n, M, 700)
    temps, seed, plan = np.tile(ladder(k, 26.0, 2.6), M), 0x5A4ED300, (2, 3)
    ref = truth(J, hs, k, seed, temps, plan, exchange=False)
    one = engine_run(sg, J, hs, k, seed, temps, plan, options=rs_options(W), exchange=False)
    assert ran(one, "sweep_dense_rs<"), one["kernels"]
    assert_same(one, ref)
    parts = []
    for r0 in (0, R // 2):
        with sg.AnnealEngine(0) as e:
            e.set_options(rs_options(W))
            e.set_dense_shared(J, hs)
            e.init_replicas(R // 2, seed=seed, R_global=R, replica0=r0)
            e.set_temperatures(temps[r0:r0 + R // 2])
            tr = []
            for ns in plan:
                tr.append(e.sweep(ns, energy_trace=True)["energy_trace"])
                assert e.last_kernel().startswith("sweep_dense_rs<"), e.last_kernel()
            bests = [e.best(r) for r in range(R // 2)]
            parts.append((np.concatenate(tr), e.spins(), e.stats()[0].copy(), e.energies().copy(),
                          np.asarray([b[0] for b in bests]), np.stack([b[1] for b in bests])))
    assert np.array_equal(np.concatenate([p[0] for p in parts], axis=1), np.concatenate(one["traces"]))
    for i, key in ((1, "spins"), (2, "acc"), (3, "energy"), (4, "best_e"), (5, "best_s")):
        assert np.array_equal(np.concatenate([p[i] for p in parts]), one[key]), key


def test_autotune_times_the_windows_for_a_shared_batch(sg):
    """Option "row_shared" = 2 (default): sga_autotune times W = 256 / 512 / 1024 as it does for one model; whichever
    form it keeps, the run continues on the oracle's chain."""
    n, M, k = 1100, 2, 3
    J, hs = pm1(n, 27), int_fields(n, M, 1000)
    temps, seed = np.tile(ladder(k, 50.0, 5.0), M), 0x5A4ED350
    ref = truth(J, hs, k, seed, temps, (2, 2), exchange=False)
    with sg.AnnealEngine(0) as e:
        e.set_dense_shared(J, hs)
        e.init_replicas(M * k, seed=seed)
        e.set_ladder(temps, n_ladders=M)
        a = e.sweep(2, energy_trace=True)["energy_trace"]
        assert e.last_kernel().startswith("sweep_dense_kernel<"), e.last_kernel()  # (not before the autotuner)
        e.autotune()
        forms = {key for key in e.autotune_table(forms=True) if key.startswith("row-shared:")}
        assert forms == {"row-shared:W256", "row-shared:W512", "row-shared:W1024"}, forms
        b = e.sweep(2, energy_trace=True)["energy_trace"]
        assert e.last_kernel().startswith(("sweep_dense_rs<", "sweep_dense_kernel<")), e.last_kernel()
        assert np.array_equal(a, ref["traces"][0]) and np.array_equal(b, ref["traces"][1])
        assert np.array_equal(e.spins(), ref["spins"]) and np.array_equal(e.energies(), ref["energy"])
        assert np.array_equal(e.stats()[0], ref["acc"])


# ----------------------------------------------------------------------------- 4. matrix-core energies
def energy_instance():
    """M = 4, k = 8: 32 replicas, the threshold of the all-replica pass; integer J, half-integer h in model 2."""
    n, M, k = 200, 4, 8
    J = int_couplings(n, 19, 3)
    hs = int_fields(n, M, 800, 2)
    hs[2] = (np.random.RandomState(9).randint(-5, 6, n) / 2.0).astype(np.float32)
    assert np.any(hs[2] != np.rint(hs[2])) and np.all(hs[0] == np.rint(hs[0]))
    return n, M, k, J, hs


def test_matrix_core_energies(sg):
    n, M, k, J, hs = energy_instance()
    R, seed = M * k, 0x5A4ED400
    probs = [oracle.Problem(J=J, h=hs[m]) for m in range(M)]
    spins = np.concatenate([oracle.init_spins(n, k, seed, replica0=m * k) for m in range(M)])
    r = 2 * k + 3  # a replica of the half-integer model
    flipped = spins.copy()
    flipped[r] = -flipped[r]

    def want(s):
        return np.concatenate([oracle.energy(probs[m], s[m * k:(m + 1) * k]) for m in range(M)]).astype(np.float64)

    assert want(spins)[r] != want(flipped)[r] and len(set(want(spins)[m * k] for m in range(M))) == M
    seen = {}
    for mode in (1, 0):  # option "batched_energy": the matrix-core pass | the per-replica kernels
        with sg.AnnealEngine(0) as e:
            e.set_option("batched_energy", mode)
            e.set_dense_shared(J, hs)
            e.init_replicas(R, seed=seed)
            assert np.array_equal(e.spins(), spins)
            first = e.energies().copy()
            e.set_spins(r, flipped[r])
            second = e.energies().copy()
            e.recompute_energies()
            third = e.energies().copy()
            seen[mode] = (first, second, third)
        assert np.array_equal(first, want(spins)), mode
        assert np.array_equal(second, want(flipped)) and np.array_equal(third, want(flipped)), mode
    for a, b in zip(seen[1], seen[0]):
        assert np.array_equal(a, b)


# ----------------------------------------------------------------------------- 5. cached fields
@pytest.mark.parametrize("cache", ["on", "auto"])
@pytest.mark.parametrize("batched", [1, 0])
def test_cached_fields(sg, cache, batched):
    n, M, k, J, hs = energy_instance()
    # AUTO at this size starts on the row kernels and looks at the counters after 4 and after 12 sweeps: the third call
    # finds the cold replicas of every ladder below the break-even and runs them cached beside the hot ones
    temps, seed, plan = np.tile(ladder(k, 40.0, 0.5), M), 0x5A4ED500, ((3, 2) if cache == "on" else (4, 8, 2))
    ref = truth(J, hs, k, seed, temps, plan)
    got = engine_run(sg, J, hs, k, seed, temps, plan, cache=cache, options={"clf_batched": batched})
    assert any("sweep_clf" in kname for kname in got["kernels"]), got["kernels"]
    want = "sweep_clfb_kernel" if batched else "sweep_clf_kernel"
    if cache == "on":
        assert ran(got, want), got["kernels"]
        assert f"cached-batch(models={M} scale=2)" in got["describe"], got["describe"]
    else:
        assert any(want in kname for kname in got["kernels"]), got["kernels"]
    assert f"models={M}" in got["explain"].split(" cached=")[1], got["explain"]
    assert_same(got, ref)


def test_cached_fields_traced_sequential_call(sg):
    n, M, k, J, hs = energy_instance()
    temps, seed, ns = np.tile(ladder(k, 40.0, 0.5), M), 0x5A4ED501, 2
    u = np.random.RandomState(0).rand(M * k, ns * n).astype(np.float32)
    kw = dict(exchange=False, trace=True, replay_u=u)
    ref = truth(J, hs, k, seed, temps, [ns], site_mode=oracle.SITE_SEQUENTIAL, **kw)
    got = engine_run(sg, J, hs, k, seed, temps, [ns], cache="on", site_mode=sg._native.SITE_SEQUENTIAL, **kw)
    assert ran(got, "sweep_clf_kernel"), got["kernels"]
    assert np.array_equal(got["accept_trace"][0], ref["accept_trace"][0])
    assert np.array_equal(got["dE_trace"][0], ref["dE_trace"][0])
    assert_same(got, ref)


@pytest.mark.parametrize("cache", ["on", "auto"])
def test_cached_fields_fixed_point(sg, cache):
    """Quarter-valued J (k = 2, int32 fields) and h off the half-integers, under the two options a stacked batch needs."""
    n, M, k = 200, 4, 8
    J = sym(np.random.RandomState(23).randint(-8, 9, (n, n)) / 4.0)
    hs = np.stack([((2 * np.random.RandomState(40 + m).randint(-4, 4, n) + 1) / 4.0).astype(np.float32) for m in range(M)])
    assert np.any(4 * J % 2 != 0) and np.all(2 * hs != np.rint(2 * hs))
    # (AUTO at this size starts on the row kernels and looks at the counters after 4 and after 12 sweeps, as above)
    temps, seed, plan = np.tile(ladder(k, 30.0, 1.0), M), 0x5A4ED502, ((3, 2) if cache == "on" else (4, 8, 2))
    ref = truth(J, hs, k, seed, temps, plan)
    options = {"clf_fixed_point": 1, "batch_fixed_point": 1}
    got = engine_run(sg, J, hs, k, seed, temps, plan, cache=cache, options=options)
    assert any("sweep_clf_fx_kernel<float," in kname and "int32 fixed-point" in kname and f"models={M}," in kname
               for kname in got["kernels"]), got["kernels"]
    if cache == "on":
        assert ran(got, "sweep_clf_fx_kernel<float,"), got["kernels"]
        assert f"fixed-point models={M}" in got["explain"], got["explain"]
    assert_same(got, ref)
    # without "batch_fixed_point" the form stays refused, in the stacked batch's words
    with sg.AnnealEngine(0) as e:
        e.set_option("clf_fixed_point", 1)
        e.set_field_cache("on")
        e.set_dense_shared(J, hs)
        e.init_replicas(M * k, seed=seed)
        e.set_temperatures(temps)
        with pytest.raises(sg.AnnealingError, match="dense batches"):
            e.sweep(1)


# ----------------------------------------------------------------------------- 6. the stacked batch on the tiled J
def test_equivalence_with_the_stacked_batch(sg):
    n, M, k = 96, 3, 4
    R = M * k
    J, hs = pm1(n, 24), int_fields(n, M, 900)
    temps, seed, plan = np.tile(ladder(k, 3.0, 0.5), M), 0x5A4ED600, (2, 3)
    ref = truth(J, hs, k, seed, temps, plan)
    for cache, kernel in (("off", "sweep_dense_kernel<"), ("on", "sweep_clf")):
        a = engine_run(sg, J, hs, k, seed, temps, plan, cache=cache)
        b = engine_run(sg, J, hs, k, seed, temps, plan, cache=cache, stacked=True)
        assert ran(a, kernel) and ran(b, kernel), (a["kernels"], b["kernels"])
        assert a["scan"] == b["scan"], (a["scan"], b["scan"])
        assert a["scan"] == (sg._native.ROUTE_DENSE, scan_words(tiled(J, M), hs)), a["scan"]
        assert_same(a, ref)
        assert_same(b, ref)
        assert a["checksum"] != b["checksum"]
        assert a["checksum"] == engine_run(sg, J, hs, k, seed, temps, [1], cache=cache)["checksum"]
        assert a["describe"].replace("shared-J ", "") == b["describe"], (a["describe"], b["describe"])
    # single-site operators on a replica of the last model, a checkpoint across the two engines, a cross-model pair
    with sg.AnnealEngine(0) as ea, sg.AnnealEngine(0) as eb:
        ea.set_dense_shared(J, hs)
        eb.set_dense_batch(tiled(J, M), hs)
        for e in (ea, eb):
            e.init_replicas(R, seed=seed)
            e.set_ladder(temps, n_ladders=M)
            e.sweep(2)
        r, sites = R - 2, np.asarray([0, 5, n - 1], np.int32)
        prob = oracle.Problem(J=J, h=hs[M - 1])
        s = ea.spins(r).copy()
        assert np.array_equal(ea.local_fields(r, sites), eb.local_fields(r, sites))
        assert np.array_equal(ea.local_fields(r, sites), [oracle.local_field(prob, s, i) for i in sites])
        assert ea.flip(r, 7) == eb.flip(r, 7)
        assert ea.update(r, 11, 2.0, 0.3) == eb.update(r, 11, 2.0, 0.3)
        assert np.array_equal(ea.spins(), eb.spins()) and np.array_equal(ea.energies(), eb.energies())
        blob_a, blob_b = ea.export_state(), eb.export_state()
        ea.import_state(blob_b)
        eb.import_state(blob_a)
        ta = ea.sweep(2, energy_trace=True)["energy_trace"]
        tb = eb.sweep(2, energy_trace=True)["energy_trace"]
        assert np.array_equal(ta, tb) and np.array_equal(ea.spins(), eb.spins())
        assert np.array_equal(ea.stats()[0], eb.stats()[0])
        assert ea.exchange() == eb.exchange() and np.array_equal(ea.slot_map(), eb.slot_map())
        # a pair of slots of two models: the shared engine answers as the stacked one does, code and wording
        answers = []
        for e in (ea, eb):
            try:
                answers.append(("taken", e.exchange_pairs([(k - 1, k)], u=[0.0])))
            except sg.AnnealingError as err:
                answers.append((err.details["code"], str(err)))
        assert answers[0] == answers[1], answers
        assert np.array_equal(ea.slot_map(), eb.slot_map())


# ----------------------------------------------------------------------------- 7. refusals
def test_refusals(sg):
    n, M, k = 96, 3, 4
    J, hs = pm1(n, 25), int_fields(n, M, 950)
    with sg.AnnealEngine(0) as e:
        e.set_dense_shared(J, hs)
        with pytest.raises(sg.AnnealingError, match="R_global must be a multiple of the number of models") as err:
            e.init_replicas(M * k + 1, seed=1)
        assert err.value.details["code"] == sg._native.ERR_INVALID
        bad = hs.copy()
        bad[1, 5] = np.nan
        with pytest.raises(sg.AnnealingError, match="non-finite") as err:
            e.set_dense_shared(J, bad)
        assert err.value.details["code"] == sg._native.ERR_INVALID
        bad_J = J.copy()
        bad_J[3, 4] = bad_J[4, 3] = np.inf
        with pytest.raises(sg.AnnealingError, match="non-finite"):
            e.set_dense_shared(bad_J, hs)
        with pytest.raises(sg.AnnealingError, match="int8 storage requested"):
            e.set_dense_shared(J * 0.5, hs, storage="i8")
        with pytest.raises(sg.AnnealingError, match="bit-plane storage needs"):
            e.set_dense_shared(J * 2.0, hs, storage="t2")
    # row_shared = 1 with a half-integer h in one model: no accept table for the batch, the row kernel simply runs
    half = hs.copy()
    half[1] = (np.random.RandomState(3).randint(-3, 4, n) / 2.0).astype(np.float32)
    assert np.any(half[1] != np.rint(half[1]))
    temps, seed, plan = np.tile(ladder(k, 3.0, 0.5), M), 0x5A4ED700, (2,)
    ref = truth(J, half, k, seed, temps, plan)
    got = engine_run(sg, J, half, k, seed, temps, plan, options=rs_options(256))
    assert ran(got, "sweep_dense_kernel<"), got["kernels"]
    assert "sweep=row-shared" not in got["describe"], got["describe"]
    assert_same(got, ref)


# ----------------------------------------------------------------------------- 8. BatchProcessor
def test_batch_processor_shared_couplings(sg):
    import torch
    n = 64
    J = torch.from_numpy(pm1(n, 26))

    def models():
        out = []
        for i in range(4):
            m = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=False))
            m.set_couplings_from_matrix(J)
            m.set_external_fields(torch.from_numpy(np.random.RandomState(i).randint(-1, 2, n).astype(np.float32)))
            m.set_spins(torch.from_numpy((np.random.RandomState(90 + i).randint(0, 2, n) * 2 - 1).astype(np.float32)))
            out.append(m)
        return out

    cfg = sg.GPUAnnealerConfig(n_sweeps=40, initial_temp=6.0, final_temp=0.3, random_seed=11)
    plain = sg.BatchProcessor(cfg, sg.BatchConfig(replicas_per_model=3)).process_models_batch(models())
    bp = sg.BatchProcessor(cfg, sg.BatchConfig(replicas_per_model=3, shared_couplings=True))
    shared = bp.process_models_batch(models())
    assert "shared-J models=4" in bp.last_description, bp.last_description
    assert len(plain) == len(shared) == 4
    for a, b in zip(shared, plain):
        assert a.best_energy == b.best_energy
        assert torch.equal(a.best_configuration, b.best_configuration)
        assert a.energy_history == b.energy_history
        assert a.temperature_history == b.temperature_history
        assert a.acceptance_rate_history == b.acceptance_rate_history
        assert (a.n_sweeps, a.algorithm, a.device, a.random_seed) == (b.n_sweeps, b.algorithm, b.device, b.random_seed)
        assert 0.0 < a.acceptance_rate_history[0] < 1.0
