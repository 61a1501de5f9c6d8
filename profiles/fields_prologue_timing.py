"""The tile kernel of the row-shared fields (csrc/sweep_dense_rs.hip, rs_fields_tiles_kernel): the prologue with every
independent load in flight together (SGA_RS_TILES_PROLOGUE) and the entry loop on 32-bit offsets (SGA_RS_TILES_LEAN) against
the parent commit's library, each switch off alone and both off: what profiles/fields_prologue.json holds.
A sibling of chain_prologue_timing.py, whose cells it drives; the libraries are named by --variants (name=path,...), built
beforehand from this tree with -DSGA_RS_TILES_...=0 ("parent": the parent commit's library), and every cell runs through this
tree's Python with SGA_LIBRARY_PATH.  Every step on the device is a process of its own under its own `timeout -k 10`, and the
first one that fails ends the run.

  --parts a,b,...  ab      alternating `bench.py --gpus 1 --steps 50 --warmup 10`, --runs of "parent" and "new"; the default
                           invocation three each; --dump-outputs of both compared array for array
                   trace   `rocprofv3 --kernel-trace --stats`, a run of its own per library at two groups: fields and chain
                           per launch in the timed regime (sweeps 5-25) as average, minimum and maximum
                   pmc     `rocprofv3 --pmc` SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_LDS of the
                           tile kernel per launch, a run of its own per library, no tracing beside it
                   fit     the fields launch alone: one group, W = 1024, 128 | 256 | 512 | 1024 replicas, a kernel trace per
                           shape and library; launch time = a + b R by least squares, the intercept a recorded
                   cells   C2a's instance at G = 2 and 1 (W = 1024), event-timed ms per sweep, --cell-runs alternating runs
                           of every library
                   by      bystanders, "parent" and "new", medians of --cell-runs alternating runs: W = 512 and 256, 256
                           replicas, Glauber, the binary grid (J = +-1/4), "row_shared_fields" = 1 over one general plane
                           (ternary J) and three (|J| <= 7) -- and bench.py --workload c3 | c4 | c5, and the autotuner's
                           row-shared table and pick on C2a
                   (a part's pieces alone: ab:steps50_warmup10, ab:default, ab:dump, by:cells, by:other, by:tune)

usage: fields_prologue_timing.py --variants parent=...,new=...,prologue0=...,lean0=...,alloff=... [--parts ...]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "fields_prologue.json")
COUNTERS = ["SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_INSTS_LDS"]
WARMUP, STEPS, N = 5, 20, 10000
FIT_R = (128, 256, 512, 1024)


def last_json(text):
    return json.loads(next(ln for ln in text.splitlines()[::-1] if ln.startswith("{")))


def env_of(lib):
    env = dict(os.environ)
    env["SGA_LIBRARY_PATH"] = os.path.abspath(lib)
    return env


def step_on_device(cmd, env, limit=300, cwd=None):
    """One process under its own time limit; anything but a clean exit ends the whole run."""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, capture_output=True, text=True, cwd=cwd)
    if p.returncode != 0:
        raise SystemExit(f"{cmd}: exit {p.returncode} -- stopping here\n{p.stderr[-800:]}")
    return p.stdout


def drive(R, G, W, kind):
    """C2a's steps on one engine (kind: c2a | grid -- J = +-1/4 | glauber | tern | a7 -- the tiles forced over general planes |
    tune -- the autotuner's table instead of the steps); one JSON line."""
    sys.path.insert(0, ROOT)
    import spin_glass_anneal_rl_amd as sg
    rng = np.random.RandomState(7)
    if kind == "tern":
        A = rng.randint(-1, 2, (N, N), dtype=np.int8) * (rng.randint(0, 100, (N, N), dtype=np.int8) < 45)
    elif kind == "a7":
        A = rng.randint(-7, 8, (N, N), dtype=np.int8)
    else:
        A = rng.randint(0, 2, (N, N), dtype=np.int8) * 2 - 1
    A = np.triu(A.astype(np.int8), 1)
    J = (A + A.T).astype(np.float32) * np.float32(0.25 if kind == "grid" else 1.0)
    hi, lo = (2.5, 0.025) if kind == "grid" else (10.0, 0.1)
    with sg.AnnealEngine(0) as e:
        if kind != "tune":
            e.set_option("row_shared", 1)
            e.set_option("row_shared_window", W)
            e.set_option("row_shared_grid", 1 if kind == "grid" else 0)
            e.set_replica_groups(G)
        if kind in ("tern", "a7"):
            e.set_option("row_shared_fields", 1)
        e.set_tuning(sweeps_per_launch=1)
        if kind == "glauber":
            e.set_update_rule(sg._native.RULE_GLAUBER)
        e.set_dense(J, np.zeros(N, np.float32), storage="f32")
        e.init_replicas(R, seed=11)
        e.set_ladder(np.asarray([hi * (lo / hi) ** (i / max(R - 1, 1)) for i in range(R)]))
        if kind == "tune":
            ms = e.autotune()
            e.sweep(1)
            print(json.dumps({"autotune_ms": ms, "table": {str(k): v for k, v in e.autotune_table(forms=True).items()},
                              "kernel": e.last_kernel()}, default=str))
            return
        done = 0

        def step():
            nonlocal done
            e.sweep(1)
            done += 1
            if done % 10 == 0:
                e.exchange(count=False)
        for _ in range(WARMUP):
            step()
        e.energies()
        e.enable_timing(True)
        e.kernel_time(reset=True)
        t0 = time.perf_counter()
        for _ in range(STEPS):
            step()
        e.energies()
        wall = time.perf_counter() - t0
        launches, kernel_ms = e.kernel_time(reset=True)
        print(json.dumps({"R": R, "G": G, "W": W, "kind": kind, "ms_per_step_wall": wall * 1e3 / STEPS,
                          "ms_per_sweep_events": kernel_ms / max(launches, 1), "kernel": e.last_kernel(),
                          "checksum": float(np.asarray(e.energies()).sum())}))


def drive_cmd(R, G, W=1024, kind="c2a"):
    return [sys.executable, os.path.abspath(__file__), "--drive", str(R), str(G), str(W), kind]


def profiled(cmd, env, rocprof_args, pattern):
    with tempfile.TemporaryDirectory() as d:
        out = step_on_device(["rocprofv3"] + rocprof_args + ["-d", d, "--output-format", "csv", "--"] + cmd, env, limit=500)
        table = list(csv.reader(open(glob.glob(os.path.join(d, "**", pattern), recursive=True)[0])))
    return last_json(out), table


def trace_cell(lib, R, G):
    """Fields and chain per launch over the timed regime (launch order is sweep order per stream)."""
    res, trace = profiled(drive_cmd(R, G), env_of(lib), ["--kernel-trace", "--stats"], "*kernel_trace.csv")
    col = {h: i for i, h in enumerate(trace[0])}
    rows = sorted(((int(r[col["Start_Timestamp"]]), int(r[col["End_Timestamp"]]), r[col["Kernel_Name"]])
                   for r in trace[1:] if "sga::rs_" in r[col["Kernel_Name"]]), key=lambda x: x[0])
    out = {"ms_per_sweep_events": res["ms_per_sweep_events"], "kernel": res["kernel"]}
    for part in ("rs_chain_kernel", "rs_fields_tiles_kernel"):
        mine = [r for r in rows if "sga::" + part in r[2]]
        us = np.asarray([(b - a) / 1e3 for a, b, _ in mine[WARMUP * len(mine) // (WARMUP + STEPS):]])
        out[part] = {"launches": len(us), "avg_us": float(us.mean()), "min_us": float(us.min()), "max_us": float(us.max())}
    return out


def pmc_cell(lib, G):
    _, rows = profiled(drive_cmd(1024, G), env_of(lib), ["--pmc"] + COUNTERS, "*counter_collection.csv")
    col = {h: i for i, h in enumerate(rows[0])}
    disp = {}
    for r in rows[1:]:
        if "sga::rs_fields_tiles_kernel" in r[col["Kernel_Name"]]:
            disp.setdefault(int(r[col["Dispatch_Id"]]), {})[r[col["Counter_Name"]]] = float(r[col["Counter_Value"]])
    ids = sorted(disp)
    ids = ids[WARMUP * len(ids) // (WARMUP + STEPS):]
    tot = {c + "_per_launch": sum(disp[i].get(c, 0.0) for i in ids) / len(ids) for c in COUNTERS}
    tot["dispatches"] = len(ids)
    tot["wait_any_share"] = tot["SQ_WAIT_ANY_per_launch"] / tot["SQ_WAVE_CYCLES_per_launch"]
    return tot


def bench(lib, extra, dump=None):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(extra) + (["--dump-outputs", dump] if dump else [])
    res = last_json(step_on_device(cmd, env_of(lib), limit=600, cwd=ROOT))
    return res["ms_per_step"], res.get("roofline", {}).get("kernel_instantiation")


def headline(base, mine):
    """The criterion: this build's slowest run ahead of the parent's fastest by at least three times the parent's own spread."""
    spread = max(base) - min(base)
    return {"parent_spread_ms": spread, "parent_fastest_minus_new_slowest_ms": min(base) - max(mine),
            "wins": bool(min(base) - max(mine) > 0 and min(base) - max(mine) >= 3 * spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab,trace,pmc,fit,cells,by")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cell-runs", type=int, default=3)
    ap.add_argument("--variants", default="")
    ap.add_argument("--profile-variants", default="", help="the libraries of trace, pmc and fit (default: all)")
    ap.add_argument("--drive", nargs=4, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.drive:
        return drive(int(a.drive[0]), int(a.drive[1]), int(a.drive[2]), a.drive[3])
    libs = dict(v.split("=") for v in a.variants.split(",") if v)
    pair = {k: libs[k] for k in ("parent", "new")}
    merged = json.load(open(OUT)) if os.path.exists(OUT) else {}

    def save():
        json.dump(merged, open(OUT, "w"), indent=1)

    def cells(shapes, which, into):
        for R, G, W, kind in shapes:
            key = f"R{R}_G{G}_W{W}_{kind}"
            cell = merged.setdefault(into, {}).setdefault(key, {})
            for _ in range(a.cell_runs):  # (the libraries alternate inside a round)
                for name, lib in which.items():
                    res = last_json(step_on_device(drive_cmd(R, G, W, kind), env_of(lib)))
                    c = cell.setdefault(name, {"events_ms": [], "wall_ms": []})
                    c["events_ms"].append(res["ms_per_sweep_events"])
                    c["wall_ms"].append(res["ms_per_step_wall"])
                    c.update(kernel=res["kernel"], checksum=res["checksum"])
                    print(into, key, name, res["ms_per_sweep_events"], flush=True)
                    save()
            for name in which:
                cell[name]["median_events_ms"] = float(np.median(cell[name]["events_ms"]))
                cell[name]["same_checksum_as_parent"] = cell[name]["checksum"] == cell["parent"]["checksum"]
            save()

    parts = a.parts.split(",")
    ab = merged.setdefault("ab_c2a", {})
    for tag, extra, runs in (("steps50_warmup10", ["--steps", "50", "--warmup", "10"], a.runs), ("default", [], 3)):
        if "ab" in parts or "ab:" + tag in parts:
            ms, kern = {t: [] for t in pair}, {}
            for _ in range(runs):
                for t in pair:
                    v, kern[t] = bench(pair[t], extra)
                    ms[t].append(v)
                    print("ab", tag, t, v, flush=True)
            ab[tag] = dict(headline(ms["parent"], ms["new"]), ms_per_step=ms, kernel=kern)
            save()
    if "ab" in parts or "ab:dump" in parts:
        with tempfile.TemporaryDirectory() as d:
            for t in pair:
                bench(pair[t], ["--steps", "20", "--warmup", "5"], dump=os.path.join(d, t))
            names = sorted(os.listdir(os.path.join(d, "parent")))
            same = names == sorted(os.listdir(os.path.join(d, "new"))) and all(
                np.array_equal(np.load(os.path.join(d, "parent", f)), np.load(os.path.join(d, "new", f))) for f in names)
        ab.update(dumped_arrays=names, dumped_arrays_equal=bool(same))
        print("ab", json.dumps(ab), flush=True)
        save()
    prof = {k: libs[k] for k in a.profile_variants.split(",") if k} or libs
    if "trace" in parts:
        for name, lib in prof.items():
            merged.setdefault("trace_c2a_W1024_G2", {})[name] = trace_cell(lib, 1024, 2)
            print("trace", name, json.dumps(merged["trace_c2a_W1024_G2"][name]), flush=True)
            save()
    if "pmc" in parts:
        for name, lib in prof.items():
            merged.setdefault("pmc_tiles_c2a_W1024_G2", {})[name] = pmc_cell(lib, 2)
            print("pmc", name, json.dumps(merged["pmc_tiles_c2a_W1024_G2"][name]), flush=True)
            save()
    if "fit" in parts:
        for name, lib in prof.items():
            us = [trace_cell(lib, R, 1)["rs_fields_tiles_kernel"]["avg_us"] for R in FIT_R]
            b, a0 = np.polyfit(np.asarray(FIT_R, float), np.asarray(us), 1)
            merged.setdefault("fit_fields_G1_W1024", {})[name] = {"replicas": list(FIT_R), "avg_us": us, "intercept_us": float(a0),
                                                                  "us_per_replica": float(b)}
            print("fit", name, json.dumps(merged["fit_fields_G1_W1024"][name]), flush=True)
            save()
    if "cells" in parts:
        cells([(1024, 2, 1024, "c2a"), (1024, 1, 1024, "c2a")], libs, "cells")
    if "by" in parts or "by:cells" in parts:
        cells([(1024, 2, 512, "c2a"), (1024, 2, 256, "c2a"), (256, 2, 1024, "c2a"), (1024, 2, 1024, "glauber"), (1024, 2, 1024, "grid"),
               (1024, 2, 1024, "tern"), (1024, 2, 1024, "a7")], pair, "bystanders")
    if "by" in parts or "by:other" in parts:
        for wl in ("c3", "c4", "c5"):
            ms = {t: [] for t in pair}
            for _ in range(3):
                for t in pair:
                    ms[t].append(bench(pair[t], ["--workload", wl])[0])
            merged.setdefault("other_workloads", {})[wl] = {"ms_per_step": ms, "median": {k: float(np.median(v)) for k, v in ms.items()}}
            print(wl, json.dumps(merged["other_workloads"][wl]), flush=True)
            save()
    if "by" in parts or "by:tune" in parts:
        for t in pair:
            merged.setdefault("autotune_c2a", {})[t] = last_json(step_on_device(drive_cmd(1024, 0, 0, "tune"), env_of(pair[t]), limit=500))
            print("tune", t, json.dumps(merged["autotune_c2a"][t]), flush=True)
            save()


if __name__ == "__main__":
    main()
