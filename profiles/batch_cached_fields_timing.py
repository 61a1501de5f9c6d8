"""Cached local fields for many-model dense batches (sga_set_dense_batch + sga_set_field_cache): ms per sweep of the
cached form (ON), of AUTO and of the BASELINE -- the library of the commit before batches were served, built as a
variant (profiles/build_variant.sh in a checkout of that commit) and loaded through SGA_LIBRARY_PATH, field cache off:
the row-per-proposal kernels every batch ran on -- written to profiles/batch_cached_fields.json.

Each (library, mode) runs in a process of its own (a library is loaded once per process); the runs ALTERNATE, `--reps`
times, on the same box, and the spread between the repetitions of one cell is recorded beside its mean.  All lines are
+-1 couplings (int8 rows, as the engine picks them), integer h:

  batch_processor   M = 32 models, k = 1 replica each, n in {256, 1024, 4096, 10^4}, the default SA schedule of
                    GPUAnnealerConfig (geometric, 10 -> 0.01, 1000 sweeps): sweeps 0..10, 50..60, 500..510, whole run
  ladders           M = 32, k = 32, n = 2000, 10 -> 0.1 per model, exchange every 10 sweeps: sweeps 5..25 and 100..110
  tiny              M = 1024, k = 1, n = 128, the SA schedule: sweeps 0..10, 500..510, whole run
  one_model         n = 10^4, 1024 replicas, 10 -> 0.1, sweeps 5..25, field cache ON and OFF: the one-model kernels of
                    the new build against the baseline's ("not slower" beyond the spread)

Every cell records the acceptance in the timed window; final energies are compared across all cells of a line.
Kernel statistics: a separate run `rocprofv3 --kernel-trace --stats -f csv -d <dir> -- python
profiles/batch_cached_fields_timing.py --worker on --quick --out <file>` (profiles/batch_cached_fields_kernel_stats.csv).
usage: batch_cached_fields_timing.py --baseline <libsga of the parent commit> [--reps 2] [--quick] [--no-write]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "batch_cached_fields.json")


def ladder(k, tmax, tmin):
    return np.asarray([tmax * (tmin / tmax) ** (i / max(k - 1, 1)) for i in range(k)])


def sa_schedule(sg, n_sweeps=1000):
    cfg = sg.GPUAnnealerConfig(n_sweeps=n_sweeps)
    sch = sg.TemperatureScheduler.create_schedule(cfg.schedule_type, cfg.initial_temp, cfg.final_temp, cfg.n_sweeps,
                                                  **cfg.schedule_params)
    return np.maximum(np.asarray([sch.update(s) for s in range(n_sweeps)]), 1e-10)


def pm1_stack(torch, M, n, seed):
    g = torch.Generator("cuda").manual_seed(seed)
    J = torch.empty((M, n, n), dtype=torch.float32, device="cuda")
    for m in range(M):
        U = torch.triu((torch.randint(0, 2, (n, n), device="cuda", generator=g) * 2 - 1).float(), 1)
        J[m] = U + U.T
    return J, torch.randint(-1, 2, (M, n), device="cuda", generator=g).float()


def timed(torch, e, n, R, windows, run_piece, total):
    """Walk sweeps [0, total) in the pieces the windows cut; {window: ms per sweep, acceptance}."""
    cuts = sorted({0, total, *[x for w in windows for x in w]})
    lines = {}
    t_all = 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        torch.cuda.synchronize()
        acc0 = e.stats()[0].copy()
        t0 = time.perf_counter()
        run_piece(a, b)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        t_all += dt
        if (a, b) in windows:
            d = (e.stats()[0] - acc0).astype(np.float64)
            lines[f"{a}..{b}"] = {"ms_per_sweep": dt / (b - a) * 1e3, "acceptance_rate": float(d.sum()) / (float(R) * n * (b - a)),
                                  "hottest_replica_acceptance": float(d.max()) / (n * (b - a)), "kernel": e.last_kernel()}
    lines[f"whole_run_0..{total}"] = {"ms_per_sweep": t_all / total * 1e3, "seconds": t_all}
    return lines


def one_model_line(torch, sg, mode):
    """One model, the kernels every one-model user runs: n = 10^4, 1024 replicas on a 10 -> 0.1 ladder."""
    n, R = 10000, 1024
    J, h = pm1_stack(torch, 1, n, 5)
    with sg.AnnealEngine(0) as e:
        e.set_field_cache(mode)
        e.set_dense(J[0], h[0], storage="i8")
        del J
        e.init_replicas(R, seed=42)
        e.set_ladder(ladder(R, 10.0, 0.1))
        res = timed(torch, e, n, R, [(5, 25)] if mode == "on" else [(0, 2)], lambda a, b: e.sweep(b - a), 25 if mode == "on" else 2)
        res["final_energies"] = e.energies().tolist()
    torch.cuda.empty_cache()
    return {f"one_model_n{n}_R{R}": res}


def worker(mode, quick, one_model_only=False):
    import torch
    import spin_glass_anneal_rl_amd as sg
    out = {"library": sg._native.library_path(), "version": sg._native.lib().sga_version(), "mode": mode}
    sched = sa_schedule(sg)

    def sa_line(M, n, windows, total):
        J, h = pm1_stack(torch, M, n, 7 + n)
        with sg.AnnealEngine(0) as e:
            e.set_field_cache(mode)
            e.set_dense_batch(J, h)
            del J
            e.init_replicas(M, seed=42)
            # (pieces of 10 sweeps, BatchProcessor's record_interval)
            def piece(a, b):
                for lo in range(a, b, 10):
                    e.sweep(min(lo + 10, b) - lo, sched=sched[lo:min(lo + 10, b)])
            res = timed(torch, e, n, M, windows, piece, total)
            res["final_energies_checksum"] = float(np.sum(e.energies()))
            res["final_energies"] = e.energies().tolist()
            res["describe"] = e.describe()
        torch.cuda.empty_cache()
        return res

    if one_model_only:
        return dict(out, **one_model_line(torch, sg, mode))
    total = 200 if quick else 1000
    sa_windows = [(0, 10), (50, 60)] if quick else [(0, 10), (50, 60), (500, 510)]
    for n in ((1024,) if quick else (256, 1024, 4096, 10000)):
        out[f"batch_processor_M32_k1_n{n}"] = sa_line(32, n, sa_windows, total)
    if not quick:
        out["tiny_M1024_k1_n128"] = sa_line(1024, 128, [(0, 10), (500, 510)], total)
    # ladders: one ladder per model, exchange every 10 sweeps
    M, k, n = 32, 32, 2000
    J, h = pm1_stack(torch, M, n, 99)
    with sg.AnnealEngine(0) as e:
        e.set_field_cache(mode)
        e.set_dense_batch(J, h)
        del J
        e.init_replicas(M * k, seed=42)
        e.set_ladder(np.tile(ladder(k, 10.0, 0.1), M), n_ladders=M)

        def piece(a, b):
            for lo in range(a, b):
                e.sweep(1)
                if (lo + 1) % 10 == 0:
                    e.exchange(count=False)
        res = timed(torch, e, n, M * k, [(5, 25)] if quick else [(5, 25), (100, 110)], piece, 25 if quick else 110)
        res["final_energies"] = e.energies().tolist()
        res["describe"] = e.describe()
        out[f"ladders_M{M}_k{k}_n{n}"] = res
    torch.cuda.empty_cache()
    if mode in ("on", "off") and not quick:
        out.update(one_model_line(torch, sg, mode))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="libsga.so of the commit before batches were served (profiles/build_variant.sh)")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--worker", help="run one mode (off | on | auto) with the library loaded and print / write its lines")
    ap.add_argument("--one-model-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        res = worker(a.worker, a.quick, a.one_model_only)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f)
        else:
            print(json.dumps(res, indent=1))
        return
    if not a.baseline or not os.path.exists(a.baseline):
        sys.exit("--baseline <library of the parent commit> is required")
    cells = [("baseline_off", a.baseline, "off"), ("new_on", None, "on"), ("new_auto", None, "auto"), ("new_off", None, "off"),
             ("baseline_on_one_model", a.baseline, "on")]
    runs = {c[0]: [] for c in cells}
    fd, tmp = tempfile.mkstemp(suffix=".json")
    os.close(fd)
    for rep in range(a.reps):  # alternating: baseline, on, auto, off, baseline, ...
        for name, lib, mode in cells:
            env = dict(os.environ)
            env.pop("SGA_LIBRARY_PATH", None)
            if lib:
                env["SGA_LIBRARY_PATH"] = os.path.abspath(lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--out", tmp] + (["--quick"] if a.quick else []) + \
                  (["--one-model-only"] if name == "baseline_on_one_model" else [])
            proc = subprocess.run(cmd, env=env, timeout=900)
            if proc.returncode != 0:  # (nothing more is started on the device after a failed cell)
                sys.exit(f"cell {name} (repetition {rep}) failed with status {proc.returncode}")
            with open(tmp) as f:
                runs[name].append(json.load(f))
            print(f"rep {rep} {name} done", flush=True)
    os.remove(tmp)
    import torch
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
           "note": "ms per sweep, wall clock around synchronised calls; mean over the alternating repetitions, spread = (max - min) / mean"}
    lines = [k for k in runs["new_on"][0] if isinstance(runs["new_on"][0][k], dict)]
    for line in lines:
        entry = {}
        ref_e = None
        for name in runs:
            if line not in runs[name][0]:
                continue
            if name == "baseline_on_one_model" and not line.startswith("one_model"):
                continue  # (the baseline refuses ON for a batch: that cell exists for the one-model line only)
            cell = {}
            for w in runs[name][0][line]:
                if not isinstance(runs[name][0][line][w], dict):
                    continue
                ms = [r[line][w]["ms_per_sweep"] for r in runs[name]]
                cell[w] = dict(runs[name][0][line][w], ms_per_sweep=float(np.mean(ms)), ms_per_sweep_runs=ms,
                               spread=float((max(ms) - min(ms)) / np.mean(ms)))
            e_fin = [r[line]["final_energies"] for r in runs[name]]
            if not line.startswith("one_model"):
                ref_e = ref_e if ref_e is not None else e_fin[0]
                assert all(x == ref_e for x in e_fin), f"final energies differ: {line} {name}"
            cell["describe"] = runs[name][0][line].get("describe")
            entry[name] = cell
        if not line.startswith("one_model"):
            entry["final_energies_equal_in_every_cell"] = True
            entry["final_energies_checksum"] = float(np.sum(ref_e))
            ratios = {}
            for w in entry["new_on"]:
                if isinstance(entry["new_on"][w], dict) and w in entry["baseline_off"]:
                    b = entry["baseline_off"][w]["ms_per_sweep"]
                    ratios[w] = {"baseline_over_on": b / entry["new_on"][w]["ms_per_sweep"],
                                 "baseline_over_auto": b / entry["new_auto"][w]["ms_per_sweep"]}
            entry["speedup"] = ratios
        out[line] = entry
    print(json.dumps(out, indent=1))
    if not a.no_write:
        with open(OUT, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
