"""Fixed-point cached local fields for ragged CSR batches (engine options "ragged_field_cache" and "clf_fixed_point"
together, version >= 1300): the streaming ragged form (both options 0 -- the kernel such batches ran before, the same
binary path) against the fixed-point cached form under SGA_FIELD_CACHE_ON and AUTO (both options 1), written to
profiles/ragged_fixed_point.json.  Needs a GPU; there is no fallback.

Cells
  realgrid    64 sparse models, n in [1000, 6000], mean degree 8, real-valued J on a 2^-6 grid in (0, 2] with random
              signs, h = 0: int32 fields, k = 6.  8 replicas per model, 200 sweeps of the default SA schedule (3.0 -> 0.1)
  tsp         TSP instances of 20, 25, ... 60 cities through encoders.tsp_csr (n = cities^2 = 400 ... 3600 spins, rows of
              4 (cities - 1) = 76 ... 236 entries, random points in the unit square scaled by 100, real-valued
              distances: int64 fields), 8 replicas per model, 200 sweeps of the default schedule type from 100 to 1
Every form runs twice, the forms alternating (streaming, on, auto, streaming, on, auto) in one process after a short
warm-up of each.  Per run: kernel time from the engine's events (sga_enable_timing) and wall time, for the whole run
and for the windows of sweeps [0, 5), [5, 25), [25, 100), [100, 200), with the acceptance of each window; final spins,
energies and every replica's best energy of every run are compared with the first streaming run's and recorded as equal (or not).
A difference between two forms counts only where the two runs of one form do not overlap the two runs of the other
("outside_spread").
usage: ragged_fixed_point_timing.py [--only realgrid|tsp] [--out FILE] [--no-write]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import spin_glass_anneal_rl_amd as sg  # noqa: E402
from spin_glass_anneal_rl_amd import _native as N  # noqa: E402
from spin_glass_anneal_rl_amd import encoders  # noqa: E402
from spin_glass_anneal_rl_amd.gpu_annealer import GPUAnnealerConfig  # noqa: E402
from spin_glass_anneal_rl_amd.temperature_scheduler import TemperatureScheduler  # noqa: E402

OUT = os.path.join(HERE, "ragged_fixed_point.json")
WINDOWS = [(0, 5), (5, 25), (25, 100), (100, 200)]
FORMS = [("streaming", 0, "off"), ("cached_on", 1, "on"), ("cached_auto", 1, "auto")]  # (name, both options, field cache)
K, SWEEPS = 8, 200


def schedule(initial, final, sweeps=SWEEPS):
    cfg = GPUAnnealerConfig(n_sweeps=sweeps, initial_temp=initial, final_temp=final)
    s = TemperatureScheduler.create_schedule(cfg.schedule_type, cfg.initial_temp, cfg.final_temp, sweeps, **cfg.schedule_params)
    return np.maximum(np.asarray([s.update(i) for i in range(sweeps)]), 1e-10)


def realgrid_cell():
    rng = np.random.RandomState(11)
    probs, sizes = [], []
    for _ in range(64):
        n = int(rng.randint(1000, 6001))
        e = rng.randint(0, n, (4 * n, 2))
        e = np.unique(np.sort(e[e[:, 0] != e[:, 1]], axis=1), axis=0)  # undirected edges, no loops, no duplicates
        v = (rng.randint(1, 129, len(e)) * (rng.randint(0, 2, len(e)) * 2 - 1)).astype(np.float32) * np.float32(2.0 ** -6)
        rows = np.concatenate([e[:, 0], e[:, 1]])
        cols = np.concatenate([e[:, 1], e[:, 0]])
        vals = np.concatenate([v, v])
        order = np.lexsort((cols, rows))
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
        probs.append((rowptr, cols[order].astype(np.int32), vals[order].astype(np.float32), np.zeros(n, np.float32)))
        sizes.append(n)
    deg = float(np.mean([p[0][-1] / (len(p[0]) - 1) for p in probs]))
    return probs, schedule(3.0, 0.1), {"models": len(probs), "n_range": [min(sizes), max(sizes)], "mean_degree": deg,
                                       "J": "m 2^-6, m in 1..128, random sign", "schedule": "default SA schedule 3.0 -> 0.1"}


def tsp_cell():
    rng = np.random.RandomState(12)
    probs, cities = [], []
    for c in range(20, 61, 5):
        xy = rng.rand(c, 2) * 100.0
        d = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1))
        rowptr, colidx, val, h, _ = encoders.tsp_csr(d)
        probs.append((rowptr.numpy().astype(np.int32), colidx.numpy().astype(np.int32), val.numpy().astype(np.float32),
                      h.numpy().astype(np.float32)))
        cities.append(c)
    rows = [int(np.diff(p[0]).max()) for p in probs]
    return probs, schedule(100.0, 1.0), {"models": len(probs), "cities": cities, "row_entries": [min(rows), max(rows)],
                                         "schedule": "default schedule type 100 -> 1"}


def run(probs, temps, option, mode, seed=3, warm=False):
    M = len(probs)
    sizes = np.asarray([len(p[0]) - 1 for p in probs])
    per_sweep = float(K * sizes.sum())
    with sg.AnnealEngine(0) as e:
        e.set_option("ragged_field_cache", option)
        e.set_option("clf_fixed_point", option)
        e.set_csr_batch(probs)
        e.set_field_cache(mode)
        e.init_replicas(M * K, seed=seed)
        if warm:
            e.sweep(3, sched=temps[:3])
            return None
        e.enable_timing(True)
        e.kernel_time(reset=True)
        out = {"windows": [], "describe": e.describe()}
        acc0 = e.stats()[0]
        t_run = time.perf_counter()
        for lo, hi in WINDOWS:
            t0 = time.perf_counter()
            e.sweep(hi - lo, sched=temps[lo:hi])
            acc1 = e.stats()[0]  # (synchronises)
            wall = time.perf_counter() - t0
            launches, ms = e.kernel_time(reset=True)
            out["windows"].append({"sweeps": [lo, hi], "kernel_ms_per_sweep": ms / (hi - lo), "wall_ms_per_sweep": 1e3 * wall / (hi - lo),
                                   "launches": launches, "kernel": e.last_kernel(),
                                   "acceptance_mean": float((acc1 - acc0).sum() / (per_sweep * (hi - lo))),
                                   "acceptance_hottest": float(((acc1 - acc0) / (np.repeat(sizes, K) * float(hi - lo))).max())})
            acc0 = acc1
        out["wall_s"] = time.perf_counter() - t_run
        out["kernel_ms"] = float(sum(w["kernel_ms_per_sweep"] * (w["sweeps"][1] - w["sweeps"][0]) for w in out["windows"]))
        out["attempts_per_s_kernel"] = per_sweep * SWEEPS / (out["kernel_ms"] * 1e-3)
        out["final"] = (e.spins(), e.energies(), np.asarray([e.best(r, with_spins=False)[0] for r in range(M * K)]))
    return out


def pair(values):
    a = [float(v) for v in values]
    return {"runs": a, "mean": float(np.mean(a)), "spread_rel": float((max(a) - min(a)) / np.mean(a))}


def cell(name, build):
    probs, temps, shape = build()
    for _, option, mode in FORMS:
        run(probs, temps, option, mode, warm=True)
    runs = {f[0]: [] for f in FORMS}
    for _ in range(2):
        for form, option, mode in FORMS:
            runs[form].append(run(probs, temps, option, mode))
    ref = runs["streaming"][0]["final"]
    report = {"shape": {**shape, "replicas_per_model": K, "sweeps": SWEEPS}, "forms": {}}
    equal = True
    for form, rr in runs.items():
        same = all(np.array_equal(r["final"][0], ref[0]) and np.array_equal(r["final"][1], ref[1]) and np.array_equal(r["final"][2], ref[2])
                   for r in rr)
        equal = equal and same
        report["forms"][form] = {
            "final_spins_energies_and_best_equal_to_streaming": bool(same), "describe": rr[0]["describe"],
            "kernel_ms": pair(r["kernel_ms"] for r in rr), "wall_s": pair(r["wall_s"] for r in rr),
            "attempts_per_s_kernel": pair(r["attempts_per_s_kernel"] for r in rr),
            "windows": [{"sweeps": w["sweeps"], "kernel": w["kernel"], "launches": w["launches"],
                         "acceptance_mean": w["acceptance_mean"], "acceptance_hottest": w["acceptance_hottest"],
                         "kernel_ms_per_sweep": pair(r["windows"][i]["kernel_ms_per_sweep"] for r in rr),
                         "wall_ms_per_sweep": pair(r["windows"][i]["wall_ms_per_sweep"] for r in rr)}
                        for i, w in enumerate(rr[0]["windows"])]}
    report["all_runs_equal"] = bool(equal)
    assert equal, "a form's final spins, energies or best energy differ from the streaming run's"
    base = report["forms"]["streaming"]
    for form in ("cached_on", "cached_auto"):
        f = report["forms"][form]

        def versus(a, b):
            out = {"streaming_over_cached": a["mean"] / b["mean"],
                   "outside_spread": bool(min(a["runs"]) > max(b["runs"]) or max(a["runs"]) < min(b["runs"]))}
            return out
        f["versus_streaming"] = {"kernel_ms": versus(base["kernel_ms"], f["kernel_ms"]), "wall_s": versus(base["wall_s"], f["wall_s"]),
                                 "windows_kernel": [versus(bw["kernel_ms_per_sweep"], fw["kernel_ms_per_sweep"])
                                                    for bw, fw in zip(base["windows"], f["windows"])]}
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["realgrid", "tsp"])
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU (there is no fallback)"
    report = {"device": torch.cuda.get_device_name(0), "library": os.path.relpath(N.library_path(), os.path.dirname(HERE)),
              "library_version": int(N.lib().sga_version()),
              "baseline": "options ragged_field_cache = clf_fixed_point = 0: the streaming ragged kernel, what these batches ran "
                          "before version 1300 (unchanged since version 600)",
              "timing": "kernel: sga_enable_timing (device events); wall: host clock around sga_sweep + counter read-back; "
                        "two alternating runs per form after a warm-up of each"}
    for name, build in (("realgrid", realgrid_cell), ("tsp", tsp_cell)):
        if args.only in (None, name):
            report[name] = cell(name, build)
            brief = {f: (v["kernel_ms"]["runs"], v["wall_s"]["runs"]) for f, v in report[name]["forms"].items()}
            print(name, report[name]["all_runs_equal"], json.dumps(brief), flush=True)
    if not args.no_write:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1, default=float)


if __name__ == "__main__":
    main()
