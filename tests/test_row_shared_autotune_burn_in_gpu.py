"""sga_autotune times each row-shared window after a burn-in at that window (csrc/sga_autotune.cpp, RS_TRIAL_BURN_IN), so
its trials run many more sweeps than before on the caller's replicas.  None of them may leak: called in the middle of a
run, the state it leaves and the chain that continues from it equal a run that never called it -- spins, energies,
accept counters, best states, sweep counter and the exchange rounds' decisions.  No assertion on times."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


def problem(n):
    rng = np.random.RandomState(300)
    A = np.triu(rng.randint(0, 2, (n, n)) * 2 - 1, 1)
    return (A + A.T).astype(np.float32), rng.randint(-1, 2, n).astype(np.float32)


def run(sg, J, h, R, temps, seed, autotune):
    out = {}
    with sg.AnnealEngine(0) as e:
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_ladder(temps)
        traces = [e.sweep(2, energy_trace=True)["energy_trace"]]
        swaps = [e.exchange()]
        if autotune:
            e.autotune()
            out["table"] = e.autotune_table(forms=True)
        out["after_autotune"] = (e.spins().copy(), e.energies().copy(), e.stats()[0].copy(), e.counters()[0],
                                 [e.best(r)[0] for r in range(R)])
        traces.append(e.sweep(3, energy_trace=True)["energy_trace"])
        swaps.append(e.exchange())
        traces.append(e.sweep(2, energy_trace=True)["energy_trace"])
        best = [e.best(r) for r in range(R)]
        out.update(trace=np.vstack(traces), swaps=swaps, spins=e.spins().copy(), energy=e.energies().copy(),
                   accepted=e.stats()[0].copy(), sweeps=e.counters()[0], slot=e.slot_map().copy(),
                   best_energy=np.asarray([b[0] for b in best]), best_spins=np.stack([b[1] for b in best]))
    return out


def test_autotune_mid_run_leaves_no_trace():
    import spin_glass_anneal_rl_amd as sg
    n, R, seed = 300, 8, 99
    J, h = problem(n)
    temps = np.asarray([10.0 * (0.1 / 10.0) ** (i / (R - 1)) for i in range(R)])
    plain = run(sg, J, h, R, temps, seed, autotune=False)
    tuned = run(sg, J, h, R, temps, seed, autotune=True)
    forms = [k for k in tuned["table"] if k.startswith("row-shared:")]
    assert forms == ["row-shared:W256", "row-shared:W512", "row-shared:W1024"], tuned["table"]
    for got, want in zip(tuned["after_autotune"], plain["after_autotune"]):
        assert np.array_equal(np.asarray(got), np.asarray(want))
    for k in ("trace", "swaps", "spins", "energy", "accepted", "sweeps", "slot", "best_energy", "best_spins"):
        assert np.array_equal(np.asarray(tuned[k]), np.asarray(plain[k])), k
    assert plain["sweeps"] == 7
    # and both are the oracle's chain up to the first exchange round
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(oracle.Problem(J=J, h=h), s, temps, 2, seed=seed)
    assert np.array_equal(plain["trace"][:2], ref["energy_trace"])
