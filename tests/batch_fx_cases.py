"""Cases and helpers of the fixed-point cached-field sweep over many-model dense batches (engine options
"clf_fixed_point" + "batch_fixed_point", csrc/sweep_clf_fx.hip): the batches, the per-model oracle that is the truth, the
engine runner and the comparisons.  Shared by tests/test_batch_fixed_point_gpu.py and tests/test_batch_fixed_point_host.py;
no test lives here."""
import numpy as np

import oracle
from scan_reference import scan_words  # noqa: F401  (the stacked scan's eight words: callers reach it through this module)

INF = float("inf")
FX_OPTIONS = {"clf_fixed_point": 1, "batch_fixed_point": 1}


def sym(A):
    """Symmetric, zero diagonal, from the upper triangle of A."""
    U = np.triu(A, 1)
    return (U + U.T).astype(np.float32)


def grid_sk(n, seed, scale=1.0):
    """SK couplings on the binary grid 2^-10: J = rint(randn 1024 scale) / 1024."""
    rng = np.random.RandomState(seed)
    return sym(np.rint(rng.randn(n, n) * 1024.0 * scale) / 1024.0)


def ladder(k, tmax, tmin):
    return np.asarray([tmax * (tmin / tmax) ** (i / max(k - 1, 1)) for i in range(k)], np.float64)


def physical_assignment(m, weight, seed):
    """m x m assignment in the physical convention (half / quarter-valued J) with integer costs and QUBO pair terms."""
    from spin_glass_anneal_rl_amd import encoders as enc
    rng = np.random.RandomState(seed)
    b = enc.assignment_ising(m, m, weight=weight, costs=rng.randint(1, 9, m * m).astype(np.float64))
    a = rng.choice(m * m, 12, replace=False)
    b.add_qubo_pair(a[:6], a[6:], 2.0 * rng.randint(1, 3, 6))  # -q / 4 couplings: -1/2, -1
    model = b.to_model(sparse=False)
    return (model.couplings.cpu().numpy().astype(np.float32), model.external_fields.cpu().numpy().astype(np.float32))


# ----------------------------------------------------------------------------- the batches (Js [M, n, n], hs [M, n])
def case_a():
    """Binary-grid SK, fp32 rows, int32, k = 10: n = 200 (below one 256-element chunk, no multiple of the row alignment)."""
    n, M = 200, 3
    Js = np.stack([grid_sk(n, 30 + m) for m in range(M)])
    hs = np.stack([(np.random.RandomState(60 + m).randn(n) * 0.7).astype(np.float32) for m in range(M)])
    return Js, hs


def case_b():
    """Model 0 carries one coupling of 2^24 beside the 2^-10 grid: int64 for the batch; model 1 alone would be int32."""
    n, M = 160, 2
    Js = np.stack([grid_sk(n, 50 + m, 0.1) for m in range(M)])
    Js[0, 3, 150] = Js[0, 150, 3] = np.float32(2.0 ** 24)
    hs = np.stack([(np.random.RandomState(70 + m).randn(n) * 0.3).astype(np.float32) for m in range(M)])
    return Js, hs


def case_c():
    """Integer J in -3..3 (int8 rows) with quarter-valued h: k = 0."""
    n, M = 300, 3
    Js = np.stack([sym(np.random.RandomState(80 + m).randint(-3, 4, (n, n)).astype(np.float32)) for m in range(M)])
    hs = np.stack([(np.random.RandomState(90 + m).randint(-8, 9, n) / 4.0).astype(np.float32) for m in range(M)])
    return Js, hs


def case_d():
    """Three 10 x 10 physical-convention assignment models: models 0 and 2 need k = 1 alone, model 1 needs k = 2."""
    parts = [physical_assignment(10, w, s) for w, s in ((5.0, 50), (2.5, 25), (5.0, 51))]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


def case_e():
    """n = 1500 at one wave: rows longer than the register batch (the streaming tail), on a model that is not model 0."""
    n, M = 1500, 2
    Js = np.stack([grid_sk(n, 110 + m) for m in range(M)])
    hs = np.stack([(np.random.RandomState(120 + m).randn(n) * 0.7).astype(np.float32) for m in range(M)])
    return Js, hs


# ----------------------------------------------------------------------------- truth: the oracle, one run per model
def oracle_batch(Js, hs, k, seed, slot_temps, plan, exchange=True, **kw):
    """Per-model oracle runs of `plan` (sweep counts) with replica0 = m k, an exchange round (one ladder per model)
    after every call."""
    M, n = Js.shape[0], Js.shape[1]
    R = M * k
    slot_temps = np.asarray(slot_temps, np.float64)
    spins = np.concatenate([oracle.init_spins(n, k, seed, replica0=m * k) for m in range(M)])
    probs = [oracle.Problem(J=Js[m], h=hs[m]) for m in range(M)]
    energy = np.concatenate([oracle.energy(probs[m], spins[m * k:(m + 1) * k]) for m in range(M)]).astype(np.float64)
    best_e, best_s = energy.copy(), spins.copy()
    acc = np.zeros(R, np.int64)
    slot = np.arange(R, dtype=np.int32)
    rep_temp = slot_temps.copy()
    traces, swaps, acc_tr, dE_tr, done = [], [], [], [], 0
    replay_u = kw.pop("replay_u", None)
    for rnd, ns in enumerate(plan):
        tr = np.zeros((ns, R))
        a_tr, d_tr = [], []
        for m in range(M):
            sl = slice(m * k, (m + 1) * k)
            s = np.ascontiguousarray(spins[sl])
            ref = oracle.sweeps(probs[m], s, rep_temp[sl], ns, seed=seed, sweep0=done, replica0=m * k, energy=energy[sl],
                                best_energy=best_e[sl], n_threads=min(k, 8),
                                replay_u=None if replay_u is None else replay_u[sl], **kw)
            spins[sl] = s
            energy[sl] = ref["energy"]
            acc[sl] += ref["n_accepted"]
            better = ref["best_energy"] < best_e[sl]
            best_s[sl][better] = ref["best_spins"][better]
            best_e[sl] = ref["best_energy"]
            tr[:, sl] = ref["energy_trace"]
            if kw.get("trace"):
                a_tr.append(ref["accept_trace"])
                d_tr.append(ref["dE_trace"])
        traces.append(tr)
        if kw.get("trace"):
            acc_tr.append(np.concatenate(a_tr))
            dE_tr.append(np.concatenate(d_tr))
        done += ns
        if exchange:
            cnt = 0
            for m in range(M):
                sl = slice(m * k, (m + 1) * k)
                view = np.ascontiguousarray(slot[sl])
                cnt += oracle.pt_exchange_round(slot_temps[sl], energy, view, seed=seed, round_=rnd, ladder=m)
                slot[sl] = view
                rep_temp[view] = slot_temps[sl]
            swaps.append(cnt)
    return dict(traces=traces, spins=spins, energy=energy, acc=acc, best_e=best_e, best_s=best_s, swaps=swaps,
                slot=slot, accept_trace=acc_tr, dE_trace=dE_tr, attempted=done * n)


def both_branches(ref, M, k):
    """A condition, from the ORACLE's counters: every model's replicas accepted something and rejected something."""
    for m in range(M):
        a = int(ref["acc"][m * k:(m + 1) * k].sum())
        assert 0 < a < k * ref["attempted"], (m, a, k * ref["attempted"])


# ----------------------------------------------------------------------------- the engine
def engine_batch(sg, Js, hs, k, seed, slot_temps, plan, cache="on", storage="auto", options=FX_OPTIONS, rule=0, exchange=True,
                 **sweep_kw):
    M = Js.shape[0]
    with sg.AnnealEngine(0) as e:
        e.set_options(options or {})
        e.set_field_cache(cache)
        e.set_dense_batch(Js, hs, storage=storage)
        e.set_update_rule(rule)
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
                    accept_trace=acc_tr, dE_trace=dE_tr)


def assert_same(got, ref):
    assert len(got["traces"]) == len(ref["traces"])
    for a, b in zip(got["traces"], ref["traces"]):
        assert np.array_equal(a, b)
    assert np.array_equal(got["spins"], ref["spins"])
    assert np.array_equal(got["energy"], ref["energy"])
    assert np.array_equal(got["acc"], ref["acc"])
    assert np.array_equal(got["best_e"], ref["best_e"])
    assert np.array_equal(got["best_s"], ref["best_s"])
    assert got["swaps"] == ref["swaps"]
    assert np.array_equal(got["slot"], ref["slot"])


def fx_ran(got, M, bits, rows="float"):
    """Every launch of the run was the batch build of sweep_clf_fx_kernel with these rows, this width and this batch."""
    return all(kname.startswith(f"sweep_clf_fx_kernel<{rows},") and f"int{bits} fixed-point" in kname and f"models={M}," in kname
               for kname in got["kernels"])
