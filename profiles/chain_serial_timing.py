"""The serial path of the row-shared chain (csrc/sweep_dense_rs.hip, rs_chain_kernel): the accept table in LDS
(SGA_RS_CHAIN_TABLE) against the parent commit, and beside it the variant libraries of what was tried with it -- the
corrections gathered one block ahead, alone ("ahead") and with the table ("table_and_ahead"), built from the source as
it stood before that part was left out: what profiles/chain_serial.json and profiles/chain_serial_kernel_stats.csv hold
(DESIGN.md 4.1h, 7).

The parent is a checkout of the parent commit with its library built (--baseline-tree).  Every cell drives C2a's instance
itself (10 000 spins, +-1 couplings, the geometric ladder T 10 -> 0.1 -- or the hot one, 200 -> 0.3 -- one sweep per call,
an exchange round every 10 steps, 5 warm-up steps, 20 timed ones, the window forced), through this tree's Python with the
library named by --variants (name=path,...; "parent" is the baseline tree's own library).  Every step on the device is a
process of its own under its own time limit, and the first one that fails ends the run.

  --parts a,b,...  trace   `rocprofv3 --kernel-trace --stats`, a run of its own per library at two groups: chain and fields
                           per launch in the timed regime (sweeps 5-25) as average, minimum and maximum
                   pmc     SQ_WAVE_CYCLES, SQ_WAIT_ANY, SQ_ACTIVE_INST_VALU, SQ_INSTS_VALU of rs_chain_kernel per wave over
                           the timed regime; a `rocprofv3 --pmc` run of its own per library, no tracing beside it
                   cells   event-timed and wall ms per step, --cell-runs runs per cell, G = 1 and 2 at 1024 and 256
                           replicas (W = 1024), W = 256 and 512 and the hot ladder at 1024 replicas and two groups; the
                           accepts per window of the timed regime from stats(); per cell and variant, whether its slowest
                           run is ahead of the baseline's fastest by 10 x the baseline's spread
                   ab      alternating plain runs of `bench.py --gpus 1 --steps 20 --warmup 5`, --runs of each tree, and
                           --dump-outputs of both compared array for array
                   other   bench.py --workload c3 | c4 | c5, three alternating runs of each tree

usage: chain_serial_timing.py --baseline-tree DIR [--parts ...] [--runs 5] [--variants table=build/libsga_table.so,...]"""
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
OUT = os.path.join(ROOT, "profiles", "chain_serial.json")
OUT_CSV = os.path.join(ROOT, "profiles", "chain_serial_kernel_stats.csv")
BENCH_ARGS = ["--gpus", "1", "--steps", "20", "--warmup", "5"]
WARMUP, STEPS, N = 5, 20, 10000
COUNTERS = ["SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_ACTIVE_INST_VALU", "SQ_INSTS_VALU"]
LADDERS = {"c2a": (10.0, 0.1), "hot": (200.0, 0.3)}
STEP_LIMIT = 300  # seconds for one process on the device


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


def step_on_device(cmd, env, cwd=None, limit=STEP_LIMIT):
    """One process under its own time limit; anything but a clean exit ends the whole run."""
    try:
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit, cwd=cwd)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"{cmd}: no end after {limit} s -- stopping here")
    if p.returncode != 0:
        raise SystemExit(f"{cmd}: exit {p.returncode} -- stopping here\n{p.stderr[-800:]}")
    return p.stdout


def drive(R, G, W, ladder):
    """C2a's steps on one engine; one JSON line."""
    sys.path.insert(0, ROOT)
    import spin_glass_anneal_rl_amd as sg
    rng = np.random.RandomState(7)
    A = np.triu((rng.randint(0, 2, (N, N), dtype=np.int8) * 2 - 1).astype(np.int8), 1)
    J = (A + A.T).astype(np.float32)
    hi, lo = LADDERS[ladder]
    with sg.AnnealEngine(0) as e:
        e.set_option("row_shared", 1)
        e.set_option("row_shared_window", W)
        e.set_tuning(sweeps_per_launch=1)
        e.set_replica_groups(G)
        e.set_dense(J, np.zeros(N, np.float32), storage="f32")
        e.init_replicas(R, seed=11)
        e.set_ladder(np.asarray([hi * (lo / hi) ** (i / max(R - 1, 1)) for i in range(R)]))  # (bench.py's ladder for c2a)
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
        acc0 = np.asarray(e.stats()[0], np.float64)
        e.enable_timing(True)
        e.kernel_time(reset=True)
        t0 = time.perf_counter()
        for _ in range(STEPS):
            step()
        e.energies()
        wall = time.perf_counter() - t0
        launches, kernel_ms = e.kernel_time(reset=True)
        per_window = (np.asarray(e.stats()[0], np.float64) - acc0) / STEPS / -(-N // W)  # per replica (slot): accepts per window
        print(json.dumps({"R": R, "G": G, "W": W, "ladder": ladder, "ms_per_step_wall": wall * 1e3 / STEPS,
                          "ms_per_sweep_events": kernel_ms / max(launches, 1), "kernel": e.last_kernel(),
                          "accepts_per_window": {"mean": float(per_window.mean()), "median": float(np.median(per_window)),
                                                 "max": float(per_window.max()), "min": float(per_window.min())},
                          "checksum": float(np.asarray(e.energies()).sum())}))


def drive_cmd(R, G, W=1024, ladder="c2a"):
    return [sys.executable, os.path.abspath(__file__), "--drive", str(R), str(G), str(W), ladder]


def profiled(cmd, env, rocprof_args, patterns):
    with tempfile.TemporaryDirectory() as d:
        out = step_on_device(["rocprofv3"] + rocprof_args + ["-d", d, "--output-format", "csv", "--"] + cmd, env, limit=500)
        tables = [list(csv.reader(open(glob.glob(os.path.join(d, "**", pat), recursive=True)[0]))) for pat in patterns]
    return last_json(out), tables


def trace_cell(lib, G):
    res, (stats, trace) = profiled(drive_cmd(1024, G), env_of(lib), ["--kernel-trace", "--stats"], ["*kernel_stats.csv", "*kernel_trace.csv"])
    col = {h: i for i, h in enumerate(trace[0])}
    rows = sorted(((int(r[col["Start_Timestamp"]]), int(r[col["End_Timestamp"]]), short_of(r[col["Kernel_Name"]]))
                   for r in trace[1:] if "sga::rs_" in r[col["Kernel_Name"]]), key=lambda x: x[0])
    out = {"ms_per_step_wall": res["ms_per_step_wall"], "ms_per_sweep_events": res["ms_per_sweep_events"], "kernel": res["kernel"]}
    for part in ("rs_chain", "rs_fields"):
        mine = [r for r in rows if r[2].startswith(part)]
        us = np.asarray([(b - a) / 1e3 for a, b, _ in mine[WARMUP * G * -(-N // 1024):]])  # (launch order is sweep order per stream)
        out[part] = {"launches": len(us), "avg_us": float(us.mean()), "min_us": float(us.min()), "max_us": float(us.max()),
                     "kernel_ms_per_sweep": float(us.sum()) / STEPS / 1e3}
    return out, stats[0], [r for r in stats[1:] if "sga::rs_" in r[0]]


def pmc_cell(lib, G):
    _, (rows,) = profiled(drive_cmd(1024, G), env_of(lib), ["--pmc"] + COUNTERS, ["*counter_collection.csv"])
    col = {h: i for i, h in enumerate(rows[0])}
    disp = {}
    for r in rows[1:]:
        if "sga::rs_chain_kernel" in r[col["Kernel_Name"]]:
            disp.setdefault(int(r[col["Dispatch_Id"]]), {})[r[col["Counter_Name"]]] = float(r[col["Counter_Value"]])
    ids = sorted(disp)[WARMUP * G * -(-N // 1024):]
    waves = len(ids) * 1024 / G  # one wave per replica of the launch's group
    tot = {c + "_per_wave": sum(disp[i].get(c, 0.0) for i in ids) / waves for c in COUNTERS}
    tot["dispatches"] = len(ids)
    tot["wait_any_share"] = tot["SQ_WAIT_ANY_per_wave"] / tot["SQ_WAVE_CYCLES_per_wave"]
    tot["valu_active_share"] = tot["SQ_ACTIVE_INST_VALU_per_wave"] / tot["SQ_WAVE_CYCLES_per_wave"]
    return tot


def plain(tree, extra=(), dump=None):
    cmd = [sys.executable, os.path.join(tree, "bench.py")] + BENCH_ARGS + list(extra) + (["--dump-outputs", dump] if dump else [])
    res = last_json(step_on_device(cmd, env_of(), cwd=tree, limit=600))
    return res["ms_per_step"], res["roofline"]["kernel_instantiation"]


def verdict(base, mine):
    """The project's criterion on one cell: the slowest run here ahead of the baseline's fastest by 10 x its spread."""
    spread = max(base) - min(base)
    return {"baseline_spread_ms": spread, "gain_ms_worst_case": min(base) - max(mine), "gain_ms_median": float(np.median(base) - np.median(mine)),
            "wins": bool(min(base) - max(mine) >= 10 * spread and min(base) > max(mine))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-tree")
    ap.add_argument("--parts", default="trace,pmc,cells,ab,other")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cell-runs", type=int, default=3)
    ap.add_argument("--variants", default="")
    ap.add_argument("--baseline-variant", default="parent", help="the variant the cells' verdicts compare against")
    ap.add_argument("--drive", nargs=4, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.drive:
        return drive(int(a.drive[0]), int(a.drive[1]), int(a.drive[2]), a.drive[3])
    trees = {"parent": os.path.abspath(a.baseline_tree) if a.baseline_tree else None, "new": ROOT}
    libs = {"new": None}
    if trees["parent"]:
        libs["parent"] = os.path.join(trees["parent"], "spin-glass-anneal-rl_amd", "csrc", "libsga.so")
    libs.update(dict(v.split("=") for v in a.variants.split(",") if v))
    merged = json.load(open(OUT)) if os.path.exists(OUT) else {}

    def save():
        json.dump(merged, open(OUT, "w"), indent=1)

    parts = a.parts.split(",")
    if "trace" in parts:
        kept = [r for r in csv.reader(open(OUT_CSV))][1:] if os.path.exists(OUT_CSV) else []
        for name, lib in libs.items():
            cell, head, body = trace_cell(lib, 2)
            print("trace", name, json.dumps(cell), flush=True)
            merged.setdefault("trace_c2a_W1024_G2", {})[name] = cell
            save()
            kept = [r for r in kept if r[0] != name] + [[name] + r for r in body]
            with open(OUT_CSV, "w", newline="") as f:
                csv.writer(f).writerows([["cell"] + head] + kept)
    if "pmc" in parts:
        for name, lib in libs.items():
            merged.setdefault("pmc_chain_c2a_W1024_G2", {})[name] = pmc_cell(lib, 2)
            print("pmc", name, json.dumps(merged["pmc_chain_c2a_W1024_G2"][name]), flush=True)
            save()
    if "cells" in parts:
        shapes = [(1024, 2, 1024, "c2a"), (1024, 1, 1024, "c2a"), (256, 2, 1024, "c2a"), (256, 1, 1024, "c2a"),
                  (1024, 2, 512, "c2a"), (1024, 2, 256, "c2a"), (1024, 2, 1024, "hot")]
        cells = merged.setdefault("cells", {})
        for R, G, W, ladder in shapes:
            key = f"R{R}_G{G}_W{W}_{ladder}"
            for _ in range(a.cell_runs):  # (the libraries alternate inside a round)
                for name, lib in libs.items():
                    res = last_json(step_on_device(drive_cmd(R, G, W, ladder), env_of(lib)))
                    c = cells.setdefault(key, {}).setdefault(name, {"events_ms": [], "wall_ms": []})
                    c["events_ms"].append(res["ms_per_sweep_events"])
                    c["wall_ms"].append(res["ms_per_step_wall"])
                    c.update(kernel=res["kernel"], accepts_per_window=res["accepts_per_window"], checksum=res["checksum"])
                    print("cell", key, name, res["ms_per_sweep_events"], res["ms_per_step_wall"], flush=True)
                    save()
            base = cells[key].get(a.baseline_variant)
            for name in libs:
                if base and name != a.baseline_variant:
                    cells[key][name]["against_" + a.baseline_variant] = verdict(base["events_ms"], cells[key][name]["events_ms"])
                    cells[key][name]["same_checksum"] = cells[key][name]["checksum"] == base["checksum"]
            print("cell", key, json.dumps({k: v.get("against_" + a.baseline_variant) for k, v in cells[key].items()}), flush=True)
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
        merged["ab_c2a"] = dict(verdict(ms["parent"], ms["new"]), ms_per_step=ms, kernel=kern, dumped_arrays=names, dumped_arrays_equal=bool(same))
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
