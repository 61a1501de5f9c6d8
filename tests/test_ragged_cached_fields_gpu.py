"""Cached local fields for ragged CSR batches (engine option "ragged_field_cache" = 1): every replica keeps the
dynamic fields D = J_m s of ITS model resident in LDS, one workgroup of four or eight waves per replica, and reads a
row on accept only.  The chain must be the streaming ragged form's, which is the CPU oracle's run on each model alone
with its global replica indices (replica0 = m k) -- bit for bit: energies, spins, counters, bests, exchanges.
Problems, ladders and the oracle follower: tests/ragged_clf_cases.py."""
import struct

import numpy as np
import pytest

import oracle
import ragged_clf_cases as rc

pytestmark = pytest.mark.gpu

K, SEED = rc.K, rc.SEED
CACHED = "sweep_clf_csr_kernel"


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def engine(sg, probs, temps, mode="on", option=1, R=None, replica0=0, R_global=None, ladder=True, seed=SEED, s0=None):
    e = sg.AnnealEngine(0)
    if option is not None:
        e.set_option("ragged_field_cache", option)  # (the first call of every test: unknown before version 1100)
    e.set_csr_batch(list(probs))
    e.set_field_cache(mode)
    Rg = len(probs) * K if R_global is None else R_global
    R = Rg if R is None else R
    e.init_replicas(R, seed=seed, R_global=Rg, replica0=replica0, s0=s0)
    if ladder and R == Rg:
        e.set_ladder(temps, n_ladders=len(probs))
    else:
        e.set_temperatures(temps[replica0:replica0 + R])
    return e


def is_cached(e):
    k = e.last_kernel()
    return k.startswith(CACHED) and "ragged" in k


def best_rows_padded(e, R, n_max):
    """[R][n_max] best-spin rows out of the export blob (header, spins [R][n_max], best spins [R][n_max], ...); the
    first block must be the spins sga_get_spins returns, which pins the offset."""
    blob = e.export_state()
    head = struct.calcsize("<Q6i2IQq")
    spins = np.frombuffer(blob, np.int8, R * n_max, head).reshape(R, n_max)
    assert np.array_equal(spins, e.spins())
    return np.frombuffer(blob, np.int8, R * n_max, head + R * n_max).reshape(R, n_max)


def assert_state(e, ob, what=""):
    """spins, energies, counters, bests of the engine against the oracle follower; padding zero"""
    R = K * len(ob.sizes)
    padded = e.spins()
    assert np.array_equal(padded, ob.padded_spins()), what
    assert np.array_equal(e.energies(), np.concatenate(ob.energy)), what
    acc, _ = e.stats()
    assert np.array_equal(acc, np.concatenate(ob.n_accepted)), what
    for r in range(R):
        m, j = divmod(r, K)
        be, bs = e.best(r)[:2]
        assert be == ob.best_energy[m][j], (what, r)
        assert np.array_equal(bs, ob.best_spins[m][j]), (what, r)
    assert np.array_equal(best_rows_padded(e, R, max(ob.sizes)), ob.padded_spins("best")), what


@pytest.mark.parametrize("name,waves,ept", [("S", 4, 1), ("L", 8, 2)])
def test_oracle_parity(sg, name, waves, ept):
    probs = rc.batch(name)
    temps = rc.ladders(probs)
    ob, trace = rc.reference(name)
    with engine(sg, probs, temps) as e:
        d = e.describe()
        assert "sweep=cached-local-fields(ragged" in d and "streaming" not in d, d
        out = e.sweep(rc.N_SWEEPS, energy_trace=True)
        k = e.last_kernel()
        assert is_cached(e) and f"<{ept} entries per thread, ragged> x {waves} wave(s)" in k, k
        assert np.array_equal(out["energy_trace"], trace)
        assert_state(e, ob, name)
        tracked = e.energies()
        e.recompute_energies()
        assert np.array_equal(e.energies(), tracked)


def test_switching_between_the_forms_and_resume(sg):
    probs = rc.batch("S")
    temps = rc.ladders(probs)
    M = len(probs)
    n_max = max(rc.sizes(probs))
    ob = rc.OracleBatch(probs, temps)
    new_spins = np.random.RandomState(5).choice(np.array([-1, 1], np.int8), rc.sizes(probs)[4])
    with engine(sg, probs, temps) as e:
        out = e.sweep(2, energy_trace=True)
        assert is_cached(e)
        assert np.array_equal(out["energy_trace"], ob.sweep(2))
        assert_state(e, ob, "first two sweeps")
        blob = e.export_state()
        # a traced sweep takes the streaming kernel; the fields are seeded anew afterwards
        out = e.sweep(1, energy_trace=True, trace=True)
        assert "sweep_csr_kernel" in e.last_kernel() and "ragged" in e.last_kernel()
        ref_trace = ob.sweep(1)
        assert np.array_equal(out["energy_trace"], ref_trace)
        assert not out["accept_trace"].reshape(M * K, n_max)[:K, 3:].any()  # model 0: three updates per sweep
        out = e.sweep(2, energy_trace=True)
        assert is_cached(e)
        assert np.array_equal(out["energy_trace"], ob.sweep(2))
        assert_state(e, ob, "after the traced sweep")
        # new spins for one replica (model 4, its middle replica), an exchange round, two more sweeps
        r = 4 * K + 1
        e.set_spins(r, new_spins)
        ob.set_spins(r, new_spins)
        assert e.exchange() == ob.exchange(0)
        assert np.array_equal(e.temperatures(), ob.temps)
        out = e.sweep(2, energy_trace=True)
        assert is_cached(e)
        assert np.array_equal(out["energy_trace"], ob.sweep(2))
        assert_state(e, ob, "after set_spins and the exchange")
    # export after the first two sweeps, import into a fresh engine, continue: the uninterrupted run without set_spins
    ob2 = rc.OracleBatch(probs, temps)
    ob2.sweep(3)
    with engine(sg, probs, temps) as e:
        e.sweep(1)  # (fields of another state are resident when the blob arrives)
        e.import_state(blob)
        out = e.sweep(1, energy_trace=True)
        assert is_cached(e)
        assert np.array_equal(out["energy_trace"][0], np.concatenate(ob2.energy))
        assert_state(e, ob2, "resumed")


def test_sharding_inside_a_model(sg):
    probs = rc.batch("S")
    temps = rc.ladders(probs)
    R = len(probs) * K
    assert R == 18
    ob, trace = rc.reference("S")
    parts = []
    for r0, Rl in ((0, 4), (4, 14)):  # the split falls inside model 1 (replicas 3..5)
        with engine(sg, probs, temps, R=Rl, replica0=r0, R_global=R, ladder=False) as e:
            out = e.sweep(rc.N_SWEEPS, energy_trace=True)
            assert is_cached(e)
            parts.append((e.spins(), e.energies(), out["energy_trace"], e.stats()[0]))
    assert np.array_equal(np.concatenate([p[0] for p in parts]), ob.padded_spins())
    assert np.array_equal(np.concatenate([p[1] for p in parts]), np.concatenate(ob.energy))
    assert np.array_equal(np.concatenate([p[2] for p in parts], axis=1), trace)
    assert np.array_equal(np.concatenate([p[3] for p in parts]), np.concatenate(ob.n_accepted))


def test_temperature_ends(sg):
    probs = rc.batch("S")
    temps = rc.ladders(probs).copy()
    temps[0::K] = np.inf  # one replica per model accepts everything ...
    temps[K - 1::K] = 0.0  # ... and one only what does not raise the energy
    ob = rc.OracleBatch(probs, temps)
    trace = ob.sweep(3)
    res = []
    for option, mode in ((1, "on"), (0, "off")):
        with engine(sg, probs, temps, mode=mode, option=option, ladder=False) as e:
            out = e.sweep(3, energy_trace=True)
            assert is_cached(e) == (option == 1)
            assert np.array_equal(out["energy_trace"], trace)
            if option == 1:
                assert_state(e, ob, "T = 0 and T = inf")
            res.append((e.spins(), e.energies(), e.stats()[0]))
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    acc = res[0][2]
    for m, n in enumerate(rc.sizes(probs)):
        assert acc[m * K] == 3 * n  # T = inf: every proposal


def test_auto_follows_the_hottest_replica(sg):
    """One launch, decided by the hottest replica of the engine at AUTO's looks (after 4, then 8, then 16 sweeps).  Cold:
    the run starts from spins the CPU has already quenched, so that every replica accepts well below the break-even
    from the first look on.  The condition on the inputs is asserted from the oracle's counters against the thresholds
    the route publishes for this engine (theta = the break-even acceptance; AUTO takes the launch onto the cached kernel
    below 0.8 theta and gives it back above 1.2 theta): every four-sweep window of the cold run lies below 0.8 theta,
    every window of the hot run above 1.2 theta."""
    import re
    probs = rc.batch("S")
    cold = rc.ladders(probs, hot=0.05, cold=0.02)
    quench = rc.OracleBatch(probs, cold)
    quench.sweep(24)
    for temps, want_cached in ((cold, True), (rc.ladders(probs), False)):
        start = [s.copy() for s in quench.spins] if want_cached else None
        ob = rc.OracleBatch(probs, temps, spins=start)
        s0 = ob.padded_spins() if want_cached else None
        with engine(sg, probs, temps, mode="auto", s0=s0) as e:
            assert "sweep=auto(ragged cached local fields" in e.describe()
            theta = float(re.search(r"cached=auto\(start=rows theta=([0-9.]+) models=6\)", e.explain_route()).group(1))
            assert 0.05 < theta < 0.5
            seen, traces, rates = [], [], []
            for _ in range(4):  # 16 sweeps: AUTO's longest interval between two looks
                before = np.concatenate(ob.n_accepted)
                traces.append(e.sweep(4, energy_trace=True)["energy_trace"])
                seen.append(is_cached(e))
                assert np.array_equal(traces[-1], ob.sweep(4))
                rates.append(((np.concatenate(ob.n_accepted) - before) / (4.0 * np.repeat(rc.sizes(probs), K))).max())
            assert not seen[0]  # nothing known yet: CSR problems start on the row kernels
            if want_cached:
                assert max(rates) < 0.8 * theta, (rates, theta)
                assert seen[1:] == [True, True, True], seen  # from the first look on
                assert "now: cached" in e.describe()
            else:
                assert min(rates) > 1.2 * theta, (rates, theta)
                assert not any(seen), seen
            assert_state(e, ob, "auto")


def _broken(kind):
    """Batch S's models 0, 1 and 3 with one model (index 1 of the batch) that keeps the batch off the int16 form."""
    n = 60
    rp, ci, v = rc.sym_sparse(n, 0.2, 900)
    h = rc.fields(n, 901)
    if kind == "real J":
        v = (v * np.float32(0.75)).astype(np.float32)
    elif kind == "row sum":
        v = (v * np.float32(4096.0)).astype(np.float32)  # rows of ~ 12 entries: integer, symmetric, sums beyond 2^15
        assert max(np.abs(v[rp[i]:rp[i + 1]]).sum() for i in range(n)) >= 2 ** 15
    elif kind == "duplicates":
        # every entry split into two halves of the same column: J is the same matrix, rows are no longer strictly sorted
        rp = (2 * rp).astype(np.int32)
        ci = np.repeat(ci, 2)
        v = np.repeat(v, 2)  # (the halves add up to 2 J: still integer, symmetric)
    elif kind == "h":
        h = (h + np.float32(0.25)).astype(np.float32)
    return (rc.batch("S")[0], (rp, ci, v, h), rc.batch("S")[1], rc.batch("S")[3])


@pytest.mark.parametrize("kind", ["real J", "row sum", "duplicates", "h"])
def test_refusals_name_the_model(sg, kind):
    from spin_glass_anneal_rl_amd import _native as N
    probs = _broken(kind)
    temps = rc.ladders(probs)
    with engine(sg, probs, temps, mode="on") as e:
        with pytest.raises(sg.AnnealingError) as ei:
            e.sweep(1)
        assert ei.value.details["code"] == N.ERR_UNSUPPORTED
        assert "model 1" in str(ei.value), str(ei.value)
        # AUTO on the same batch streams
        e.set_field_cache("auto")
        ob = rc.OracleBatch(probs, temps)
        traces = [e.sweep(4, energy_trace=True)["energy_trace"] for _ in range(2)]
        assert "sweep_csr_kernel" in e.last_kernel() and "ragged" in e.last_kernel()
        ref = ob.sweep(8)
        assert np.array_equal(np.concatenate(traces), ref)
        assert np.array_equal(e.spins(), ob.padded_spins())


def test_batch_processor_runs_the_cached_ragged_form(sg, monkeypatch):
    import torch
    from spin_glass_anneal_rl_amd.batch import BatchConfig, BatchProcessor
    from spin_glass_anneal_rl_amd.engine import AnnealEngine
    from spin_glass_anneal_rl_amd.gpu_annealer import GPUAnnealerConfig
    from spin_glass_anneal_rl_amd.ising_model import IsingModel, IsingModelConfig

    calls = {"ragged": 0, "dense": 0}
    kernels = []
    real_r, real_d, real_sweep = AnnealEngine.set_csr_batch, AnnealEngine.set_dense_batch, AnnealEngine.sweep

    def count_r(self, *a, **kw):
        calls["ragged"] += 1
        return real_r(self, *a, **kw)

    def count_d(self, *a, **kw):
        calls["dense"] += 1
        return real_d(self, *a, **kw)

    def note_sweep(self, *a, **kw):
        out = real_sweep(self, *a, **kw)
        kernels.append(self.last_kernel())
        return out

    monkeypatch.setattr(AnnealEngine, "set_csr_batch", count_r)
    monkeypatch.setattr(AnnealEngine, "set_dense_batch", count_d)
    monkeypatch.setattr(AnnealEngine, "sweep", note_sweep)
    models = []
    for i, n in enumerate([40, 75, 33, 120, 64, 51, 90]):
        m = IsingModel(IsingModelConfig(n_spins=n, use_sparse=True))
        rp, ci, v = rc.sym_sparse(n, 0.1, 300 + i)
        J = np.zeros((n, n), np.float32)
        for r in range(n):
            J[r, ci[rp[r]:rp[r + 1]]] = v[rp[r]:rp[r + 1]]
        m.set_couplings_from_matrix(torch.from_numpy(J))
        m.set_external_fields(torch.from_numpy(rc.fields(n, 400 + i, half=(i == 2))))
        models.append(m)
    res = {}
    for mode in ("on", "off"):
        cfg = GPUAnnealerConfig(n_sweeps=20, initial_temp=3.0, final_temp=0.2, random_seed=5, field_cache=mode)
        bp = BatchProcessor(cfg, BatchConfig(batch_size=4, replicas_per_model=2, ragged_field_cache=True))
        kernels.clear()
        res[mode] = bp.process_models_batch(models)
        if mode == "on":
            assert kernels and all(k.startswith(CACHED) and "ragged" in k for k in kernels), kernels[-1:]
        else:
            assert all("sweep_csr_kernel" in k for k in kernels)
    assert calls == {"ragged": 4, "dense": 0}
    for a, b in zip(res["on"], res["off"]):
        for f in a.__dataclass_fields__:
            if f == "total_time":
                continue
            x, y = getattr(a, f), getattr(b, f)
            if isinstance(x, torch.Tensor):
                assert torch.equal(x, y), f
            else:
                assert x == y, f
