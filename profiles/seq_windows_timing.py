"""Sequential windows (sga_set_sequential_windows, csrc/sweep_dense_seq.hip): kernel time per SITE_SEQUENTIAL sweep of
the windows (W = 256 | 512 | 1024) against W = 0 -- the row-per-proposal kernel sequential sweeps ran before, in the
same library -- and the split of the windows' time between product and chain, written to profiles/seq_windows.json
(DESIGN.md 4.1o, 7).

Problem: n = 10^4, one ladder 10 -> 0.1 (bench.py's C2a ladder), field cache off, random spins, Philox uniforms.
  pm1_f32 | pm1_i8 | pm1_t2   J = +-1, h in {-1, 0, 1}, in fp32, int8 and bit-plane storage
  quarter_f32                 J = +-1/4, h quarter-valued, option "row_shared_grid" = 1 (the grid form)
Replicas: 1024 for every problem; 64 and 8 as well for pm1_f32 (where does the form stop paying?).
A cell (problem, replicas) is one process.  Its arms W = 0, 256, 512, 1024 alternate, `--reps` (3) runs each, every run
on a fresh engine: `--warmup` (16) untimed sweeps, then `--sweeps` (16) timed ones; kernel time is the engine's own
(sga_enable_timing: events around every sweep launch).  Reported: the median over the runs, with min and max.  Final
spins and energies must be equal in every run of a cell: asserted.
The split: one more process per (cell, W > 0) under `rocprofv3 --kernel-trace --stats`, the same sweeps with the
engine's timing off; kernel totals by name over the whole profiled run (warm-up included).
usage: seq_windows_timing.py --time t.json        (the arms)
       seq_windows_timing.py --split s.json       (the rocprofv3 runs)
       seq_windows_timing.py --merge t.json s.json [bench.json]   (writes profiles/seq_windows.json)"""
import argparse
import csv
import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "seq_windows.json")

CELLS = [("pm1_f32", 1024), ("pm1_i8", 1024), ("pm1_t2", 1024), ("quarter_f32", 1024), ("pm1_f32", 64), ("pm1_f32", 8)]
ARMS = [0, 256, 512, 1024]
SEQ = 1  # SGA_SITE_SEQUENTIAL


def ladder(k, tmax, tmin):
    return np.asarray([tmax * (tmin / tmax) ** (i / max(k - 1, 1)) for i in range(k)])


def problem(torch, name, n):
    g = torch.Generator("cuda").manual_seed(2)
    U = torch.triu((torch.randint(0, 2, (n, n), device="cuda", generator=g, dtype=torch.int8) * 2 - 1), 1)
    J = (U + U.T).to(torch.float32)
    if name.startswith("quarter"):
        return J * 0.25, torch.randint(-8, 9, (n,), device="cuda", generator=g).float() * 0.25
    return J, torch.randint(-1, 2, (n,), device="cuda", generator=g).float()


def one_run(sg, J, h, name, R, W, warmup, sweeps, timing=True):
    with sg.AnnealEngine(0) as e:
        e.set_option("row_shared_grid", 1 if name.startswith("quarter") else 0)
        e.set_field_cache("off")
        e.set_sequential_windows(W)
        e.set_dense(J, h, storage=name.split("_")[1])
        e.init_replicas(R, seed=42)
        e.set_ladder(ladder(R, 10.0, 0.1))
        e.enable_timing(timing)
        e.sweep(warmup, site_mode=SEQ)
        if timing:
            e.kernel_time(reset=True)
        acc0 = e.stats()[0].copy()
        e.sweep(sweeps, site_mode=SEQ)
        ms = e.kernel_time(reset=True)[1] if timing else float("nan")
        d = (e.stats()[0] - acc0).astype(np.float64)
        spins, energies = e.spins(), e.energies()
        return {"W": W, "kernel_ms_per_sweep": ms / sweeps, "flips_per_proposal": float(d.sum()) / (float(R) * J.shape[0] * sweeps),
                "kernel": e.last_kernel(), "describe": e.describe(),
                "final_sha256": hashlib.sha256(np.ascontiguousarray(spins).tobytes() + np.ascontiguousarray(energies).tobytes()).hexdigest()}


def worker(name, R, arms, n, reps, warmup, sweeps, timing):
    import torch
    import spin_glass_anneal_rl_amd as sg
    torch.zeros(1, device="cuda")
    J, h = problem(torch, name, n)
    runs = []
    for rep in range(reps):  # the arms alternate: forwards, backwards, ...
        for W in (arms if rep % 2 == 0 else arms[::-1]):
            runs.append(one_run(sg, J, h, name, R, W, warmup, sweeps, timing))
            print(f"{name} R={R} W={W} run {rep}: {runs[-1]['kernel_ms_per_sweep']:.3f} ms  {runs[-1]['kernel'][:60]}", flush=True)
    return runs


def kernel_split(directory):
    """totals by kernel family from rocprofv3's kernel_stats.csv"""
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    assert len(files) == 1, files
    out = {"product_ns": 0, "chain_ns": 0, "other_ns": 0, "product_calls": 0, "chain_calls": 0, "other": {}}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            name, ns, calls = row["Name"], int(float(row["TotalDurationNs"])), int(row["Calls"])
            if "seq_product_kernel" in name:
                out["product_ns"] += ns
                out["product_calls"] += calls
                out["product_kernel"] = name
            elif "seq_chain_kernel" in name:
                out["chain_ns"] += ns
                out["chain_calls"] += calls
                out["chain_kernel"] = name
            else:
                out["other_ns"] += ns
                out["other"][name[:80]] = ns
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", metavar="JSON")
    ap.add_argument("--split", metavar="JSON")
    ap.add_argument("--merge", nargs="+", metavar="JSON")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--sweeps", type=int, default=16)
    ap.add_argument("--quick", action="store_true", help="n = 2048")
    ap.add_argument("--cells", help="comma list of NAME:R (default: all)")
    ap.add_argument("--worker", nargs=3, metavar=("NAME", "R", "ARMS"))
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    n = 2048 if a.quick else 10000
    cells = [(c.split(":")[0], int(c.split(":")[1])) for c in a.cells.split(",")] if a.cells else CELLS
    if a.worker:
        runs = worker(a.worker[0], int(a.worker[1]), [int(w) for w in a.worker[2].split(",")], n, a.reps, a.warmup, a.sweeps,
                      not a.no_timing)
        with open(a.out, "w") as f:
            json.dump(runs, f)
        return
    common = ["--warmup", str(a.warmup), "--sweeps", str(a.sweeps)] + (["--quick"] if a.quick else [])
    if a.time:
        import torch
        res = {"device": torch.cuda.get_device_name(0), "n": n, "sweeps_timed": [a.warmup, a.warmup + a.sweeps], "reps": a.reps,
               "note": "kernel ms per SITE_SEQUENTIAL sweep from the engine's events over the timed sweeps; median [min, max] over "
                       "the runs of an arm, arms alternating; W = 0 is the row-per-proposal kernel of the same library", "cells": {}}
        tmp = a.time + ".cell"
        for name, R in cells:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", name, str(R), ",".join(map(str, ARMS)), "--out", tmp,
                   "--reps", str(a.reps)] + common
            proc = subprocess.run(cmd, timeout=600)
            if proc.returncode != 0:  # (nothing more is started on the device after a failed cell)
                sys.exit(f"cell {name} R={R} failed with status {proc.returncode}")
            with open(tmp) as f:
                runs = json.load(f)
            assert len({r["final_sha256"] for r in runs}) == 1, f"final spins / energies differ between the arms: {name} R={R}"
            cell = {"final_spins_and_energies_equal_in_every_run": True, "flips_per_proposal": runs[0]["flips_per_proposal"]}
            for W in ARMS:
                ms = [r["kernel_ms_per_sweep"] for r in runs if r["W"] == W]
                first = next(r for r in runs if r["W"] == W)
                cell[f"W{W}"] = {"median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": ms,
                                 "kernel": first["kernel"], "describe": first["describe"]}
            cell["W0_over"] = {f"W{W}": cell["W0"]["median_ms"] / cell[f"W{W}"]["median_ms"] for W in ARMS if W}
            res["cells"][f"{name}_R{R}"] = cell
            with open(a.time, "w") as f:
                json.dump(res, f, indent=1)
        os.remove(tmp)
        print(json.dumps({k: {w: v[w]["median_ms"] for w in ("W0", "W256", "W512", "W1024")} for k, v in res["cells"].items()}, indent=1))
    if a.split:
        res = {}
        base = os.path.splitext(a.split)[0] + "_prof"
        for name, R in cells:
            for W in ARMS[1:]:
                d = f"{base}_{name}_R{R}_W{W}"
                shutil.rmtree(d, ignore_errors=True)
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable,
                       os.path.abspath(__file__), "--worker", name, str(R), str(W), "--out", a.split + ".cell", "--reps", "1",
                       "--no-timing"] + common
                proc = subprocess.run(cmd, timeout=600, stdout=subprocess.DEVNULL)
                if proc.returncode != 0:
                    sys.exit(f"profile of {name} R={R} W={W} failed with status {proc.returncode}")
                s = kernel_split(d)
                sweeps = a.warmup + a.sweeps
                s.update(sweeps_profiled=sweeps, product_ms_per_sweep=s["product_ns"] / 1e6 / sweeps,
                         chain_ms_per_sweep=s["chain_ns"] / 1e6 / sweeps, other_ms_per_sweep=s["other_ns"] / 1e6 / sweeps)
                res[f"{name}_R{R}_W{W}"] = s
                shutil.rmtree(d, ignore_errors=True)
                print(f"{name} R={R} W={W}: product {s['product_ms_per_sweep']:.3f} chain {s['chain_ms_per_sweep']:.3f} "
                      f"other {s['other_ms_per_sweep']:.3f} ms per sweep", flush=True)
                with open(a.split, "w") as f:
                    json.dump(res, f, indent=1)
        os.remove(a.split + ".cell")
    if a.merge:
        with open(a.merge[0]) as f:
            out = json.load(f)
        if len(a.merge) > 1:
            with open(a.merge[1]) as f:
                split = json.load(f)
            out["split_note"] = ("product / chain: kernel totals of a rocprofv3 --kernel-trace --stats run of its own over warm-up and timed "
                                 "sweeps together, per sweep; other: everything else in that process (set-time kernels, best tracking, "
                                 "the product's memset)")
            for key, s in split.items():
                cell, W = key.rsplit("_", 1)
                out["cells"][cell][W]["split"] = {k: s[k] for k in ("product_ms_per_sweep", "chain_ms_per_sweep", "other_ms_per_sweep",
                                                                     "product_calls", "chain_calls", "sweeps_profiled")}
        if len(a.merge) > 2:
            with open(a.merge[2]) as f:
                out["random_site_headline_unchanged"] = json.load(f)
        with open(OUT, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
