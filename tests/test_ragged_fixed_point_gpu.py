"""Fixed-point cached local fields for ragged CSR batches (engine options "ragged_field_cache" = 1 and "clf_fixed_point" =
1 together): batches the int16 form refuses -- real-valued J, an h off the half-integers, fields past 2^15 -- keep
D = 2^k J_m s of each replica's model resident in LDS as exact int32 | int64 at ONE batch-wide k.  The chain must be
the streaming ragged form's, which is the CPU oracle's run on each model alone with its global replica indices
(replica0 = m k) -- bit for bit: energies, spins, counters, bests, exchanges.
Problems, ladders and references: tests/ragged_fx_cases.py (oracle follower: tests/ragged_clf_cases.py)."""
import re
import struct

import numpy as np
import pytest

import oracle
import ragged_clf_cases as rc
import ragged_fx_cases as fx

pytestmark = pytest.mark.gpu

K, SEED = fx.K, fx.SEED
CACHED = "sweep_clf_csr_kernel"


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def engine(sg, probs, temps, mode="on", options=(1, 1), R=None, replica0=0, R_global=None, ladder=True, seed=SEED, s0=None):
    e = sg.AnnealEngine(0)
    e.set_option("ragged_field_cache", options[0])
    e.set_option("clf_fixed_point", options[1])
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


def is_cached(e, bits=None):
    k = e.last_kernel()
    return (k.startswith(CACHED) and "ragged" in k and "fixed-point" in k and (bits is None or f"int{bits} fixed-point" in k))


def is_streaming(e):
    return "sweep_csr_kernel" in e.last_kernel() and "ragged" in e.last_kernel()


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
    assert np.array_equal(e.spins(), ob.padded_spins()), what  # (zero past n_m)
    assert np.array_equal(e.energies(), np.concatenate(ob.energy)), what
    acc, _ = e.stats()
    assert np.array_equal(acc, np.concatenate(ob.n_accepted)), what
    for r in range(R):
        m, j = divmod(r, K)
        be, bs = e.best(r)[:2]
        assert be == ob.best_energy[m][j], (what, r)
        assert np.array_equal(bs, ob.best_spins[m][j]), (what, r)
    assert np.array_equal(best_rows_padded(e, R, max(ob.sizes)), ob.padded_spins("best")), what


@pytest.mark.parametrize("name,bits,waves,ept", [("A", 32, 4, 1), ("B", 64, 4, 1), ("C", 32, 8, 2)])
def test_oracle_parity(sg, name, bits, waves, ept):
    """On a build without the form this fails at `sweep`: "model 0: J is not integer valued"."""
    probs = fx.batch(name)
    temps = fx.ladders(probs)
    ob, trace = fx.reference(name)
    with engine(sg, probs, temps) as e:
        d = e.describe()
        assert "sweep=cached-local-fields(ragged" in d and "streaming" not in d, d
        assert f"models={len(probs)}" in d and f"int{bits} fixed-point" in d and f"k={fx.batch_k(probs)}," in d, d
        assert e.explain_route().endswith(f" cached=on(waves={waves} fields=int{bits} fixed-point models={len(probs)})")
        out = e.sweep(fx.N_SWEEPS, energy_trace=True)
        k = e.last_kernel()
        assert is_cached(e, bits) and f"<{ept} entries per thread, ragged> x {waves} wave(s)" in k, k
        assert f"k={fx.batch_k(probs)}," in k, k
        assert np.array_equal(out["energy_trace"], trace)
        assert_state(e, ob, name)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_same_chain_as_the_streaming_form(sg, name):
    probs = fx.batch(name)
    temps = fx.ladders(probs)
    res = []
    for options, mode in (((1, 1), "on"), ((0, 0), "off")):
        with engine(sg, probs, temps, mode=mode, options=options) as e:
            out = e.sweep(fx.N_SWEEPS, energy_trace=True)
            assert is_cached(e) == (mode == "on") and is_streaming(e) == (mode == "off"), e.last_kernel()
            res.append((out["energy_trace"], e.spins(), e.energies(), e.stats()[0],
                        np.asarray([e.best(r)[0] for r in range(len(probs) * K)])))
    for a, b in zip(*res):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("rule,arith", [(oracle.RULE_GLAUBER, None), (oracle.RULE_HEAT_BATH, None),
                                        (None, oracle.ARITH_F32)])
def test_rules_and_arithmetic(sg, rule, arith):
    probs = fx.batch("A")
    temps = fx.ladders(probs)
    ob, trace = fx.reference("A", rule=rule, arith=arith)
    with engine(sg, probs, temps) as e:
        if rule is not None:
            e.set_update_rule(rule)
        out = e.sweep(fx.N_SWEEPS, energy_trace=True, **({} if arith is None else {"arith": arith}))
        assert is_cached(e, 32), e.last_kernel()
        assert np.array_equal(out["energy_trace"], trace)
        assert_state(e, ob, (rule, arith))


def test_mid_run_events(sg):
    probs = fx.batch("A")
    temps = fx.ladders(probs)
    M = len(probs)
    n_max = max(rc.sizes(probs))
    ob = rc.OracleBatch(probs, temps)
    new_spins = np.random.RandomState(5).choice(np.array([-1, 1], np.int8), rc.sizes(probs)[4])
    with engine(sg, probs, temps) as e:
        out = e.sweep(2, energy_trace=True)
        assert is_cached(e, 32)
        assert np.array_equal(out["energy_trace"], ob.sweep(2))
        assert_state(e, ob, "first two sweeps")
        blob = e.export_state()
        # a traced sweep takes the streaming kernel; the fields are seeded anew afterwards
        out = e.sweep(1, energy_trace=True, trace=True)
        assert is_streaming(e), e.last_kernel()
        assert np.array_equal(out["energy_trace"], ob.sweep(1))
        assert not out["accept_trace"].reshape(M * K, n_max)[:K, 3:].any()  # model 0: three updates per sweep
        out = e.sweep(2, energy_trace=True)
        assert is_cached(e, 32)
        assert np.array_equal(out["energy_trace"], ob.sweep(2))
        assert_state(e, ob, "after the traced sweep")
        # new spins for one replica (model 4, its middle replica), then two more sweeps
        r = 4 * K + 1
        e.set_spins(r, new_spins)
        ob.set_spins(r, new_spins)
        out = e.sweep(2, energy_trace=True)
        assert is_cached(e, 32)
        assert np.array_equal(out["energy_trace"], ob.sweep(2))
        assert_state(e, ob, "after set_spins")
        # one exchange round: temperatures move, fields stay
        assert e.exchange() == ob.exchange(0)
        assert np.array_equal(e.temperatures(), ob.temps)
        out = e.sweep(2, energy_trace=True)
        assert is_cached(e, 32)
        assert np.array_equal(out["energy_trace"], ob.sweep(2))
        assert_state(e, ob, "after the exchange")
    # export after the first two sweeps, import into a fresh engine, continue: the uninterrupted run
    ob2 = rc.OracleBatch(probs, temps)
    ob2.sweep(2)
    with engine(sg, probs, temps) as e:
        e.sweep(1)  # (fields of another state are resident when the blob arrives)
        e.import_state(blob)
        out = e.sweep(2, energy_trace=True)
        assert is_cached(e, 32)
        assert np.array_equal(out["energy_trace"], ob2.sweep(2))
        assert_state(e, ob2, "resumed")


def test_sharding_inside_a_model(sg):
    probs = fx.batch("A")
    temps = fx.ladders(probs)
    R = len(probs) * K
    assert R == 15
    ob, trace = fx.reference("A")
    parts = []
    for r0, Rl in ((0, 4), (4, 11)):  # the split falls inside model 1 (replicas 3..5)
        assert r0 % K or r0 == 0
        with engine(sg, probs, temps, R=Rl, replica0=r0, R_global=R, ladder=False) as e:
            out = e.sweep(fx.N_SWEEPS, energy_trace=True)
            assert is_cached(e, 32)
            parts.append((e.spins(), e.energies(), out["energy_trace"], e.stats()[0]))
    assert np.array_equal(np.concatenate([p[0] for p in parts]), ob.padded_spins())
    assert np.array_equal(np.concatenate([p[1] for p in parts]), np.concatenate(ob.energy))
    assert np.array_equal(np.concatenate([p[2] for p in parts], axis=1), trace)
    assert np.array_equal(np.concatenate([p[3] for p in parts]), np.concatenate(ob.n_accepted))


def test_temperature_ends(sg):
    probs = fx.batch("A")
    temps = fx.ladders(probs).copy()
    temps[0::K] = np.inf  # one replica per model accepts everything ...
    temps[K - 1::K] = 0.0  # ... and one only what does not raise the energy
    ob = rc.OracleBatch(probs, temps)
    trace = ob.sweep(3)
    with engine(sg, probs, temps, ladder=False) as e:
        out = e.sweep(3, energy_trace=True)
        assert is_cached(e, 32)
        assert np.array_equal(out["energy_trace"], trace)
        assert_state(e, ob, "T = 0 and T = inf")
        acc = e.stats()[0]
    for m, n in enumerate(rc.sizes(probs)):
        assert acc[m * K] == 3 * n  # T = inf: every proposal


def test_auto_follows_the_hottest_replica(sg):
    """One launch, decided by the hottest replica against its own n_m at AUTO's looks.  Cold: the run starts from spins
    the CPU has already quenched.  The condition on the inputs is asserted from the oracle's counters against the
    thresholds the route publishes for this engine (theta: the one-model int32 fixed-point break-even; AUTO enters
    below 0.8 theta and leaves above 1.2 theta): every four-sweep window of the cold run lies below 0.8 theta, every
    window of the hot run above 1.2 theta."""
    probs = fx.batch("A")
    cold = fx.ladders(probs, hot=0.05, cold=0.02)
    quench = rc.OracleBatch(probs, cold)
    quench.sweep(24)
    for temps, want_cached in ((cold, True), (fx.ladders(probs), False)):
        start = [s.copy() for s in quench.spins] if want_cached else None
        ob = rc.OracleBatch(probs, temps, spins=start)
        s0 = ob.padded_spins() if want_cached else None
        with engine(sg, probs, temps, mode="auto", s0=s0) as e:
            assert "sweep=auto(ragged cached local fields" in e.describe() and "int32 fixed-point" in e.describe()
            theta = float(re.search(r"cached=auto\(start=rows theta=([0-9.]+) models=5\)", e.explain_route()).group(1))
            assert 0.01 < theta < 0.1  # (the fixed-point break-even: well below the int16 form's)
            seen, rates = [], []
            for _ in range(4):  # 16 sweeps: AUTO's longest interval between two looks
                before = np.concatenate(ob.n_accepted)
                tr = e.sweep(4, energy_trace=True)["energy_trace"]
                seen.append(is_cached(e, 32))
                assert seen[-1] or is_streaming(e)
                assert np.array_equal(tr, ob.sweep(4))
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


def _refused(kind):
    """(batch, index of the model that keeps it off the fixed-point form)"""
    a0, a1 = fx.batch("A")[0], fx.batch("A")[1]
    n = 60
    if kind == "f64-canonical":
        # Gaussian J over 80 binary orders of magnitude: the set bits of a row span more than 53 places
        rp, ci, v = rc.sym_sparse(n, 0.2, 910)
        rng = np.random.RandomState(911)
        J = np.zeros((n, n), np.float64)
        for r in range(n):
            J[r, ci[rp[r]:rp[r + 1]]] = 1.0
        g = np.triu(rng.randn(n, n) * 2.0 ** rng.randint(-40, 41, (n, n)), 1)
        J = np.where(J != 0, g + g.T, 0).astype(np.float32)
        return (a0, rc.dense_to_csr(J) + (rc.fields(n, 912),), a1), 1
    if kind == "duplicates":
        # every entry split into two halves of the same column: rows are no longer strictly sorted
        rp, ci, v = fx.grid_sparse(n, 0.2, 913, 5)
        return (a0, a1, ((2 * rp).astype(np.int32), np.repeat(ci, 2), np.repeat(v, 2), rc.fields(n, 914))), 2
    assert kind == "bound"
    # one model on a 2^-30 grid beside one with row sums of 2^24: 2^30 2^24 >= 2^53 at the batch-wide k
    rp, ci, v = rc.sym_sparse(20, 0.5, 915)
    fine = (rp, ci, (v * np.float32(3.0 * 2.0 ** -30)).astype(np.float32), rc.fields(20, 916))
    assert fx.lowest_bit_exponent(fine[2]) == 30
    m = 17
    J = (np.ones((m, m), np.float32) - np.eye(m, dtype=np.float32)) * np.float32(2.0 ** 20)  # rows of 16 entries
    big = rc.dense_to_csr(J) + (rc.fields(m, 917),)
    assert np.abs(big[2][big[0][0]:big[0][1]]).sum() == 2.0 ** 24
    return (a0, fine, big), 2


@pytest.mark.parametrize("kind", ["f64-canonical", "duplicates", "bound"])
def test_refusals_name_the_model(sg, kind):
    from spin_glass_anneal_rl_amd import _native as N
    probs, bad = _refused(kind)
    temps = fx.ladders(probs)
    with engine(sg, probs, temps, mode="on") as e:
        with pytest.raises(sg.AnnealingError) as ei:
            e.sweep(1)
        assert ei.value.details["code"] == N.ERR_UNSUPPORTED
        assert f"model {bad}" in str(ei.value) and "fixed point" in str(ei.value), str(ei.value)
        # AUTO on the same batch streams: the run of an engine with both options at 0
        e.set_field_cache("auto")
        tr = np.concatenate([e.sweep(4, energy_trace=True)["energy_trace"] for _ in range(2)])
        assert is_streaming(e), e.last_kernel()
        spins = e.spins()
    with engine(sg, probs, temps, mode="off", options=(0, 0)) as e:
        assert np.array_equal(e.sweep(8, energy_trace=True)["energy_trace"], tr)
        assert np.array_equal(e.spins(), spins)


def test_batch_processor_runs_the_ragged_fixed_point_form(sg, monkeypatch):
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
        rp, ci, v = fx.grid_sparse(n, 0.1, 300 + i, 3 + i % 4)
        J = np.zeros((n, n), np.float32)
        for r in range(n):
            J[r, ci[rp[r]:rp[r + 1]]] = v[rp[r]:rp[r + 1]]
        m.set_couplings_from_matrix(torch.from_numpy(J))
        m.set_external_fields(torch.from_numpy(fx.odd_fields(n, 400 + i)))
        models.append(m)
    res = {}
    for flags in (True, False):
        cfg = GPUAnnealerConfig(n_sweeps=20, initial_temp=3.0, final_temp=0.2, random_seed=5,
                                field_cache="on" if flags else "off", fixed_point_fields=flags)
        bp = BatchProcessor(cfg, BatchConfig(batch_size=4, replicas_per_model=2, ragged_field_cache=flags))
        kernels.clear()
        res[flags] = bp.process_models_batch(models)
        if flags:
            assert kernels and all(k.startswith(CACHED) and "ragged" in k and "fixed-point" in k for k in kernels), kernels[-1:]
        else:
            assert all("sweep_csr_kernel" in k for k in kernels)
    assert calls == {"ragged": 4, "dense": 0}
    for a, b in zip(res[True], res[False]):
        for f in a.__dataclass_fields__:
            if f == "total_time":
                continue
            x, y = getattr(a, f), getattr(b, f)
            if isinstance(x, torch.Tensor):
                assert torch.equal(x, y), f
            else:
                assert x == y, f
