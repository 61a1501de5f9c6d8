"""Group couplings plus a stored sparse remainder (sga_set_groups_csr, csrc/sweep_groups.hip, REST) against the
stored-coupling forms on the same chain, written to profiles/groups_rest.json.

  c4_prec     BASELINE configs[3]'s shape (500 tasks x 1 agent x 100 slots = 50 000 spins, weights assignment 100,
              capacity 50) plus chain precedence, precedence_pairs = [(t, t + 1)], at weight 80: integer remainder
              values, rows within SGA_GROUPS_MAX_REST_ROW (asserted); 1024 replicas on one 500 -> 5 ladder, an
              exchange round every 10 sweeps

Forms: "groups_rest" (this library), "csr_rows" (set_csr on the materialised couplings, one row per proposal),
"csr_cached" (set_csr with set_field_cache("on")) -- the two CSR forms in a child process on the library
--baseline-lib names (the parent commit's build, through SGA_LIBRARY_PATH) -- and "groups_no_prec": this library's
sga_set_groups on the same instance WITHOUT precedence, another chain (what the remainder costs; its final state is
not compared).  Runs alternate, --reps times; each run times sweeps 5..25 and 100..110 (kernel time from the engine's
events) and reports the final state's digest, which must agree between the three forms of the same chain.
usage: groups_rest_timing.py [--baseline-lib PATH] [--reps 2] [--only FORM] [--no-write] [--out PATH]"""
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
OUT = os.path.join(ROOT, "profiles", "groups_rest.json")
FORMS = ["groups_rest", "csr_cached", "csr_rows", "groups_no_prec"]
NEW = ("sga_set_groups", "sga_set_groups_csr")  # calls the parent's build may predate
MAX_REST_ROW = 256
R, SEED = 1024, 11


def instance(name):
    from spin_glass_anneal_rl_amd import encoders as enc
    w = {"assignment": 100.0, "capacity": 50.0}
    kw = dict(durations=np.full(500, 1.0), n_agents=1, time_horizon=100.0, time_discretization=100, objective="total_time")
    if name == "c4_prec":
        w["precedence"] = 80.0
        kw["precedence_pairs"] = [(t, t + 1) for t in range(499)]
    return enc.scheduling_ising(penalty_weights=w, **kw), (500.0, 5.0)


def run_form(name, form):
    import spin_glass_anneal_rl_amd as sg
    if form.startswith("csr") and os.environ.get("SGA_LIBRARY_PATH"):  # the parent's build predates sga_set_groups_csr
        sg._native.SYMBOLS = [s for s in sg._native.SYMBOLS if s[0] not in NEW]
    bld, (hot, cold) = instance("c4" if form == "groups_no_prec" else name)
    e = sg.AnnealEngine(0)
    if form == "groups_no_prec":
        mp, mem, c, h, _ = bld.group_structure()
        e.set_groups(bld.n, (mp, mem), c, h)
    elif form == "groups_rest":
        mp, mem, c, rest, h, _ = bld.group_rest_structure()
        lens = np.diff(rest[0])
        assert lens.max() <= MAX_REST_ROW and np.array_equal(rest[2], np.round(rest[2])), (lens.max(), "integer remainder")
        e.set_groups(bld.n, (mp, mem), c, h, rest=rest)
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
    ap.add_argument("--instances", default="c4_prec")
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
            for form in ([a.only] if a.only else FORMS):
                env = dict(os.environ)
                if form.startswith("csr") and a.baseline_lib:
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
        same_chain = {r["final_energy_digest"] for r in mine if r["form"] != "groups_no_prec"}
        assert len(same_chain) == 1, f"{name}: the forms' final states differ"
        for form in sorted({r["form"] for r in mine}):
            for cell in mine[0]["cells"]:
                v = [r["cells"][cell]["kernel_ms_per_sweep"] for r in mine if r["form"] == form]
                summary[f"{name}/{form}/{cell}"] = dict(kernel_ms_per_sweep_mean=float(np.mean(v)),
                                                        spread_ms=float(max(v) - min(v)), runs=len(v))
    doc = dict(what="sga_set_groups_csr against the stored-coupling forms, same chain (equal final states asserted), and sga_set_groups on the instance without precedence",
               baseline_library=os.path.basename(a.baseline_lib) or "same build", summary=summary, runs=runs)
    print(json.dumps(summary, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
