"""Replica groups of the row-shared sweep (csrc/sweep_dense_rs.hip, launch_sweep_dense_rs; sga_set_replica_groups) against
the parent commit: what profiles/replica_groups.json and profiles/replica_groups_kernel_stats.csv hold.

The parent is a checkout of the parent commit with its library built (--baseline-tree): its Python binds the symbols its
own library has.  Every cell drives C2a's instance itself (10 000 spins, +-1 couplings, 1024 replicas on the geometric
ladder T 10 -> 0.1, one sweep per call, an exchange round every 10 steps, 5 warm-up steps, 20 timed ones, W = 1024 forced), so that the
groups can be forced through the setter; the plain runs are bench.py's own.

  --parts a,b,...  trace   `rocprofv3 --kernel-trace --stats`, a run of its own per library and group count: chain and fields
                           per launch in the timed regime (sweeps 5-25) as average, minimum and maximum, kernel time per
                           sweep by part, and the start and end stamps of every kernel of one steady-state window (sweep
                           15, window 5) -- kernels of different groups overlap there
                   pmc     SQ_WAVE_CYCLES, SQ_WAIT_ANY, SQ_ACTIVE_INST_VALU, SQ_INSTS_VALU of rs_chain_kernel, summed over
                           the timed regime; a `rocprofv3 --pmc` run of its own, no tracing beside it
                   cells   event-timed and wall ms per step, G forced to 1, 2, 4 and the rule's choice, at 1024, 256 and
                           64 replicas, for this build and every --variants library (the other side of the priority A/B)
                   ab      alternating plain runs of `bench.py --gpus 1 --steps 20 --warmup 5`, --runs of each tree, and
                           --dump-outputs of both compared array for array
                   other   bench.py --workload c3 | c4 | c5, three alternating runs of each tree

usage: replica_groups_timing.py --baseline-tree DIR [--parts ...] [--runs 5] [--variants prio=build/libsga_prio.so,...]"""
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
OUT = os.path.join(ROOT, "profiles", "replica_groups.json")
OUT_CSV = os.path.join(ROOT, "profiles", "replica_groups_kernel_stats.csv")
BENCH_ARGS = ["--gpus", "1", "--steps", "20", "--warmup", "5"]
WARMUP, STEPS, NWIN = 5, 20, 10
COUNTERS = ["SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_ACTIVE_INST_VALU", "SQ_INSTS_VALU"]


def part_of(short):
    return ("fields" if short.startswith("rs_fields") else "chain" if short.startswith("rs_chain") else
            "planes (once)" if short.startswith("rs_planes") else "plan" if short.startswith(("rs_tile_plan", "rs_plan", "rs_scan")) else
            "pack" if short.startswith("rs_pack") else "other")


def short_of(name):
    return name.split("sga::")[1].split("(")[0].split("<")[0] if "sga::" in name else name.split("(")[0]


def last_json(text):
    return json.loads(next(ln for ln in text.splitlines()[::-1] if ln.startswith("{")))


def env_of(lib=None):
    env = dict(os.environ)
    env.pop("SGA_LIBRARY_PATH", None)
    if lib:
        env["SGA_LIBRARY_PATH"] = os.path.abspath(lib)
    return env


def drive(tree, R, G):
    """C2a's steps on one engine; one JSON line."""
    sys.path.insert(0, tree)
    import spin_glass_anneal_rl_amd as sg
    n = 10000
    rng = np.random.RandomState(7)
    A = np.triu((rng.randint(0, 2, (n, n), dtype=np.int8) * 2 - 1).astype(np.int8), 1)
    J = (A + A.T).astype(np.float32)
    with sg.AnnealEngine(0) as e:
        e.set_option("row_shared", 1)
        e.set_option("row_shared_window", 1024)
        e.set_tuning(sweeps_per_launch=1)
        if G >= 0:  # (-1: a library without the setter -- the parent)
            e.set_replica_groups(G)
        e.set_dense(J, np.zeros(n, np.float32), storage="f32")
        e.init_replicas(R, seed=11)
        e.set_ladder(np.asarray([10.0 * (0.1 / 10.0) ** (i / max(R - 1, 1)) for i in range(R)]))  # (bench.py's ladder for c2a)
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
        print(json.dumps({"R": R, "G": G, "ms_per_step_wall": wall * 1e3 / STEPS, "ms_per_sweep_events": kernel_ms / max(launches, 1),
                          "kernel": e.last_kernel(), "checksum": float(np.asarray(e.energies()).sum())}))


def drive_cmd(tree, R, G):
    return [sys.executable, os.path.abspath(__file__), "--drive", tree, str(R), str(G)]


def profiled(cmd, env, rocprof_args, patterns):
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3"] + rocprof_args + ["-d", d, "--output-format", "csv", "--"] + cmd, env=env, capture_output=True,
                           text=True, timeout=500)
        if p.returncode != 0:
            raise SystemExit(f"{cmd}: exit {p.returncode}\n{p.stderr[-800:]}")
        tables = [list(csv.reader(open(glob.glob(os.path.join(d, "**", pat), recursive=True)[0]))) for pat in patterns]
    return last_json(p.stdout), tables


def trace_cell(tree, lib, G):
    res, (stats, trace) = profiled(drive_cmd(tree, 1024, G), env_of(lib), ["--kernel-trace", "--stats"], ["*kernel_stats.csv", "*kernel_trace.csv"])
    col = {h: i for i, h in enumerate(trace[0])}
    rows = sorted(((int(r[col["Start_Timestamp"]]), int(r[col["End_Timestamp"]]), short_of(r[col["Kernel_Name"]]),
                    r[col["Stream_Id"]] if "Stream_Id" in col else r[col["Queue_Id"]]) for r in trace[1:] if "sga::rs_" in r[col["Kernel_Name"]]
                   or "sga::update_best" in r[col["Kernel_Name"]]), key=lambda x: x[0])
    groups = max(G, 1) if G > 0 else (4 if "groups=4" in res["kernel"] else 2 if "groups=2" in res["kernel"] else 1)
    out = {"ms_per_step_wall": res["ms_per_step_wall"], "ms_per_sweep_events": res["ms_per_sweep_events"], "kernel": res["kernel"]}
    per_launch, per_sweep = {}, {}
    for part in ("chain", "fields", "plan"):
        mine = [r for r in rows if part_of(r[2]) == part]
        per = groups * (NWIN if part != "plan" else 1)
        timed = mine[WARMUP * per:]  # (launch order is sweep order inside every stream; the sort is by start)
        us = np.asarray([(b - a) / 1e3 for a, b, _, _ in timed])
        if len(us):
            per_launch[part] = {"launches": len(us), "avg_us": float(us.mean()), "min_us": float(us.min()), "max_us": float(us.max())}
            per_sweep[part] = float(us.sum()) / STEPS / 1e3
    out["us_per_launch_timed"], out["kernel_ms_per_sweep_timed"] = per_launch, per_sweep
    # one steady-state window: the fields and chain launches of sweep 15, window 5, of every group
    chains = [r for r in rows if part_of(r[2]) == "chain"]
    fields = [r for r in rows if part_of(r[2]) == "fields"]
    at = (15 * NWIN + 5) * groups
    win = sorted(fields[at:at + groups] + chains[at:at + groups], key=lambda x: x[0])
    t0 = win[0][0]
    out["steady_window_us"] = [{"kernel": k, "stream": s, "start": (a - t0) / 1e3, "end": (b - t0) / 1e3} for a, b, k, s in win]
    out["steady_window_overlap"] = bool(any(x[1] > y[0] for x, y in zip(win, win[1:])))
    head, body = stats[0], [r for r in stats[1:] if "sga::rs_" in r[0] or "sga::update_best" in r[0]]
    return out, head, body


def pmc_cell(tree, lib, G):
    _, (rows,) = profiled(drive_cmd(tree, 1024, G), env_of(lib), ["--pmc"] + COUNTERS, ["*counter_collection.csv"])
    col = {h: i for i, h in enumerate(rows[0])}
    disp = {}
    for r in rows[1:]:
        if "sga::rs_chain_kernel" in r[col["Kernel_Name"]]:
            disp.setdefault(int(r[col["Dispatch_Id"]]), {})[r[col["Counter_Name"]]] = float(r[col["Counter_Value"]])
    ids = sorted(disp)[WARMUP * NWIN * max(G, 1):]
    tot = {c: sum(disp[i].get(c, 0.0) for i in ids) for c in COUNTERS}
    tot["dispatches"] = len(ids)
    if tot["SQ_WAVE_CYCLES"]:
        tot["wait_any_share"] = tot["SQ_WAIT_ANY"] / tot["SQ_WAVE_CYCLES"]
        tot["valu_active_share"] = tot["SQ_ACTIVE_INST_VALU"] / tot["SQ_WAVE_CYCLES"]
    return tot


def plain(tree, extra=(), dump=None):
    cmd = [sys.executable, os.path.join(tree, "bench.py")] + BENCH_ARGS + list(extra) + (["--dump-outputs", dump] if dump else [])
    p = subprocess.run(cmd, env=env_of(), capture_output=True, text=True, timeout=600, cwd=tree)
    if p.returncode != 0:
        raise SystemExit(f"{cmd}: exit {p.returncode}\n{p.stderr[-800:]}")
    res = last_json(p.stdout)
    return res["ms_per_step"], res["roofline"]["kernel_instantiation"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-tree")
    ap.add_argument("--parts", default="trace,pmc,cells,ab,other")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--variants", default="")
    ap.add_argument("--trace-groups", default="1,0")
    ap.add_argument("--cell-replicas", default="1024,256,64")
    ap.add_argument("--drive", nargs=3, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.drive:
        return drive(a.drive[0], int(a.drive[1]), int(a.drive[2]))
    if a.baseline_tree:
        a.baseline_tree = os.path.abspath(a.baseline_tree)
    trees = {"parent": a.baseline_tree, "new": ROOT}
    variants = dict(v.split("=") for v in a.variants.split(",") if v)
    merged = json.load(open(OUT)) if os.path.exists(OUT) else {}

    def save():
        json.dump(merged, open(OUT, "w"), indent=1)

    parts = a.parts.split(",")
    if "trace" in parts:
        kept = [r for r in csv.reader(open(OUT_CSV))][1:] if os.path.exists(OUT_CSV) else []
        cells = ([("parent", a.baseline_tree, None, -1)] if a.baseline_tree else []) + [(f"new_G{g}", ROOT, None, int(g)) for g in a.trace_groups.split(",")]
        for name, tree, lib, G in cells:
            cell, head, body = trace_cell(tree, lib, G)
            print("trace", name, json.dumps(cell), flush=True)
            merged.setdefault("trace_c2a_W1024", {})[name] = cell
            save()
            kept = [r for r in kept if r[0] != name] + [[name] + r for r in body]
            with open(OUT_CSV, "w", newline="") as f:
                csv.writer(f).writerows([["cell"] + head] + kept)
    if "pmc" in parts:
        for name, tree, G in ([("parent", a.baseline_tree, -1)] if a.baseline_tree else []) + [("new_G0", ROOT, 0)]:
            merged.setdefault("pmc_chain_c2a_W1024", {})[name] = pmc_cell(tree, None, G)
            print("pmc", name, json.dumps(merged["pmc_chain_c2a_W1024"][name]), flush=True)
            save()
    if "cells" in parts:
        for lname, lib in [("new", None)] + list(variants.items()):
            for R in (int(r) for r in a.cell_replicas.split(",")):
                for G in (1, 2, 4, 0):
                    p = subprocess.run(drive_cmd(ROOT, R, G), env=env_of(lib), capture_output=True, text=True, timeout=400)
                    if p.returncode != 0:
                        raise SystemExit(f"cell {lname} R={R} G={G}: exit {p.returncode}\n{p.stderr[-800:]}")
                    res = last_json(p.stdout)
                    merged.setdefault("cells", {}).setdefault(lname, {}).setdefault(f"R{R}", {})[f"G{G}"] = res
                    print("cell", lname, json.dumps(res), flush=True)
                    save()
    if "ab" in parts:
        ms, kern = {t: [] for t in trees}, {}
        for _ in range(a.runs):
            for t in trees:
                v, kern[t] = plain(trees[t])
                ms[t].append(v)
                print("ab", t, v, flush=True)
        with tempfile.TemporaryDirectory() as d:
            for t in trees:
                plain(trees[t], dump=os.path.join(d, t))
            names = sorted(os.listdir(os.path.join(d, "parent")))
            same = names == sorted(os.listdir(os.path.join(d, "new"))) and all(
                np.array_equal(np.load(os.path.join(d, "parent", f)), np.load(os.path.join(d, "new", f))) for f in names)
        spread = max(ms["parent"]) - min(ms["parent"])
        merged["ab_c2a"] = {"ms_per_step": ms, "kernel": kern, "parent_spread_ms": spread, "gain_ms_worst_case": min(ms["parent"]) - max(ms["new"]),
                            "criterion_10x_spread_met": bool(min(ms["parent"]) - max(ms["new"]) >= 10 * spread),
                            "dumped_arrays": names, "dumped_arrays_equal": bool(same)}
        print("ab", json.dumps(merged["ab_c2a"]), flush=True)
        save()
    if "other" in parts:
        for wl in ("c3", "c4", "c5"):
            ms = {t: [] for t in trees}
            for _ in range(3):
                for t in trees:
                    ms[t].append(plain(trees[t], extra=["--workload", wl])[0])
            merged.setdefault("other_workloads", {})[wl] = {"ms_per_step": ms, "median": {k: float(np.median(v)) for k, v in ms.items()}}
            print(wl, json.dumps(merged["other_workloads"][wl]), flush=True)
            save()


if __name__ == "__main__":
    main()
