"""Implicit cardinality-group couplings (sga_set_groups, csrc/sweep_groups.hip) against the stored-coupling forms on the
same chain, written to profiles/groups.json.

  c4          BASELINE configs[3] as bench.py builds it (500 tasks x 100 slots = 50 000 spins, 600 groups, K_i = 2),
              1024 replicas on one 500 -> 5 ladder, an exchange round every 10 sweeps
  assignment  the 100 x 100 assignment instance (10 000 spins, 200 groups), 1024 replicas, 10 -> 0.1

Forms: "groups" (this library), "csr_rows" (set_csr, one row per proposal) and "csr_cached" (set_csr with
set_field_cache("on")).  The two CSR forms run in a child process on the library --baseline-lib names (the parent
commit's build, through SGA_LIBRARY_PATH), so that the baseline is the code as it stood.  Runs alternate
groups / csr_cached / csr_rows, --reps times; each run times sweeps 5..25 and 100..110 (kernel time from the engine's
events, wall time around the same calls) and reports the final energies' digest, which must agree in every cell.
Kernel statistics come from a separate run under `rocprofv3 --kernel-trace --stats -- python profiles/groups_timing.py
--only groups --no-write`.
usage: groups_timing.py [--baseline-lib PATH] [--reps 2] [--only FORM] [--instances c4,assignment] [--no-write] [--out PATH]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "groups.json")
R, SEED = 1024, 11


def instance(name):
    from spin_glass_anneal_rl_amd import encoders as enc
    if name == "c4":
        kw = dict(durations=np.full(500, 1.0), n_agents=1, time_horizon=100.0, time_discretization=100,
                  objective="total_time", penalty_weights={"assignment": 100.0, "capacity": 50.0})
        return enc.scheduling_ising(**kw), (500.0, 5.0)
    return enc.assignment_ising(100, 100), (10.0, 0.1)


def run_form(name, form):
    import spin_glass_anneal_rl_amd as sg
    if form != "groups" and os.environ.get("SGA_LIBRARY_PATH"):  # the parent's build predates sga_set_groups
        sg._native.SYMBOLS = [s for s in sg._native.SYMBOLS if s[0] != "sga_set_groups"]
    bld, (hot, cold) = instance(name)
    e = sg.AnnealEngine(0)
    if form == "groups":
        mp, mem, c, h, _ = bld.group_structure()
        e.set_groups(bld.n, (mp, mem), c, h)
    else:
        if form == "csr_cached":
            e.set_field_cache("on")
        else:
            e.set_csr_storage("f32")  # bench.py's graded C4 line
        e.set_csr(*bld.to_csr(), bld.fields())
    e.init_replicas(R, seed=SEED)
    e.set_ladder(np.geomspace(hot, cold, R), 1)
    e.enable_timing(True)
    cells, done = {}, 0

    def advance(to):
        nonlocal done
        while done < to:
            step = min(to, (done // 10 + 1) * 10) - done
            e.sweep(step)
            done += step
            if done % 10 == 0:
                e.exchange(count=False)

    for lo, hi in ((5, 25), (100, 110)):
        advance(lo)
        e.energies()
        e.kernel_time(reset=True)
        acc0 = e.stats()[0].sum()
        t0 = time.perf_counter()
        advance(hi)
        e.energies()  # (synchronises)
        wall = time.perf_counter() - t0
        launches, ms = e.kernel_time(reset=True)
        k = hi - lo
        cells[f"sweeps_{lo}_{hi}"] = dict(kernel_ms_per_sweep=ms / k, wall_ms_per_sweep=1e3 * wall / k,
                                          attempts_per_s=R * bld.n * k / (ms * 1e-3), launches=int(launches),
                                          acceptance=float(e.stats()[0].sum() - acc0) / (R * bld.n * k))
    out = dict(form=form, instance=name, n=bld.n, R=R, kernel=e.last_kernel(), describe=e.describe(), cells=cells,
               final_energy_digest=hashlib.sha256(e.energies().tobytes() + e.spins().tobytes()).hexdigest()[:16],
               library=os.path.basename(sg._native.library_path()))
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default="")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--instances", default="c4,assignment")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child", nargs=2, metavar=("INSTANCE", "FORM"))
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(run_form(*a.child)))
        return
    runs = []
    for name in a.instances.split(","):
        for rep in range(a.reps):
            for form in ([a.only] if a.only else ["groups", "csr_cached", "csr_rows"]):
                env = dict(os.environ)
                if form != "groups" and a.baseline_lib:
                    env["SGA_LIBRARY_PATH"] = os.path.abspath(a.baseline_lib)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, form], env=env,
                                   capture_output=True, text=True, timeout=900)
                if p.returncode != 0:
                    print(p.stdout[-2000:], p.stderr[-2000:])
                    sys.exit(p.returncode)  # (nothing more is started on the GPU after a failed run)
                r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
                r["rep"] = rep
                runs.append(r)
                print(name, form, rep, {k: round(v["kernel_ms_per_sweep"], 4) for k, v in r["cells"].items()},
                      r["final_energy_digest"], flush=True)
    summary = {}
    for name in a.instances.split(","):
        mine = [r for r in runs if r["instance"] == name]
        assert len({r["final_energy_digest"] for r in mine}) == 1, f"{name}: the forms' final states differ"
        for form in sorted({r["form"] for r in mine}):
            for cell in mine[0]["cells"]:
                v = [r["cells"][cell]["kernel_ms_per_sweep"] for r in mine if r["form"] == form]
                summary[f"{name}/{form}/{cell}"] = dict(kernel_ms_per_sweep_mean=float(np.mean(v)),
                                                        spread_ms=float(max(v) - min(v)), runs=len(v))
    doc = dict(what="sga_set_groups against the stored-coupling forms, same chain (equal final states asserted)",
               baseline_library=os.path.basename(a.baseline_lib) or "same build", summary=summary, runs=runs)
    print(json.dumps(summary, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
