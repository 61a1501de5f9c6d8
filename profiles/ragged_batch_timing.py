"""Ragged many-model CSR batches (sga_set_csr_batch): the three measurements of the feature, written to
profiles/ragged_batch.json.  Kernel times come from the engine's own event timing (sga_enable_timing); every timed
shape is swept first to warm it up.  Kernel statistics come from a separate run of this script under
`rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/ragged_batch_timing.py --only overhead --no-write`
(its top_kernels table: profiles/ragged_batch_kernel_stats.csv, durations in us).

  1. overhead   C3 shape (n = 10 000, degree ~32, 4096 replicas), both engines held to the one-update narrow form
                (option csr_updates_per_step = 0): sga_set_csr against a ragged engine with M = 1
  2. copies     M = 16 copies of that problem, 256 replicas each: attempts/s and the structure's footprint
  3. mixed      64 seeded sparse +-1 models, n in [1000, 6000], mean degree 8, replicas_per_model = 8, 200 sweeps,
                through BatchProcessor.process_models_batch on the ragged path and on the densified by-size path
                (the same models handed over dense); wall clock including set-up, and the ragged kernel's attempts/s
                next to its imbalance bound mean(n_m) / max(n_m)
usage: ragged_batch_timing.py [--only overhead|copies|mixed] [--no-write]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import spin_glass_anneal_rl_amd as sg  # noqa: E402
from spin_glass_anneal_rl_amd.batch import BatchConfig, BatchProcessor  # noqa: E402
from spin_glass_anneal_rl_amd.gpu_annealer import GPUAnnealerConfig  # noqa: E402
from spin_glass_anneal_rl_amd.ising_model import IsingModel, IsingModelConfig  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ragged_batch.json")


def ladder(R, tmax=3.0, tmin=0.3):
    return np.asarray([tmax * (tmin / tmax) ** (i / max(R - 1, 1)) for i in range(R)])


def timed_sweeps(e, sweeps, warm=3):
    e.sweep(warm)  # warm-up of this shape: LDS limits, code objects, caches
    e.enable_timing(True)
    e.kernel_time(reset=True)
    e.sweep(sweeps)
    launches, ms = e.kernel_time(reset=True)
    e.enable_timing(False)
    return ms, launches


def overhead(sweeps=20):
    rp, ci, v = bench.make_sparse_instance(10000, 16, 3)
    n, R = 10000, 4096
    h = np.zeros(n, np.float32)
    out = {}
    for name in ("set_csr", "set_csr_batch_M1"):
        with sg.AnnealEngine(0) as e:
            e.set_option("csr_updates_per_step", 0)
            if name == "set_csr":
                e.set_csr(rp, ci, v, h)
            else:
                e.set_csr_batch([(rp, ci, v, h)])
            e.init_replicas(R, seed=1)
            e.set_temperatures(np.tile(ladder(64), R // 64))
            ms, launches = timed_sweeps(e, sweeps)
            out[name] = {"attempts_per_s": R * n * sweeps / (ms * 1e-3), "kernel_ms": ms, "launches": launches,
                         "sweeps": sweeps, "kernel": e.last_kernel(), "describe": e.describe()}
    out["ratio_batch_over_csr"] = out["set_csr_batch_M1"]["attempts_per_s"] / out["set_csr"]["attempts_per_s"]
    out["shape"] = {"n": n, "nnz": int(ci.size), "R": R, "option": "csr_updates_per_step=0"}
    return out


def copies(sweeps=20):
    rp, ci, v = bench.make_sparse_instance(10000, 16, 3)
    n, M, k = 10000, 16, 256
    h = np.zeros(n, np.float32)
    with sg.AnnealEngine(0) as e:
        e.set_csr_batch([(rp, ci, v, h)] * M)
        e.init_replicas(M * k, seed=2)
        e.set_ladder(np.tile(ladder(k), M), n_ladders=M)
        ms, launches = timed_sweeps(e, sweeps)
        entry_bytes = 8 * M * int(ci.size)  # (column, value) per entry
        return {"M": M, "replicas_per_model": k, "n": n, "attempts_per_s": M * k * n * sweeps / (ms * 1e-3),
                "kernel_ms": ms, "launches": launches, "sweeps": sweeps,
                "footprint_bytes": {"entries": entry_bytes, "rowptr": 8 * (M * n + 1), "h": 4 * M * n,
                                    "one_structure_entries": 8 * int(ci.size), "ratio_to_one": M},
                "kernel": e.last_kernel(), "describe": e.describe()}


def mixed_models(count=64, seed=11, dense=False):
    rng = np.random.RandomState(seed)
    models, sizes = [], []
    for i in range(count):
        n = int(rng.randint(1000, 6001))
        rows = np.repeat(np.arange(n), 4)  # mean degree 8 after symmetrisation
        cols = rng.randint(0, n, rows.size)
        keep = rows != cols
        lo, hi = np.minimum(rows[keep], cols[keep]), np.maximum(rows[keep], cols[keep])
        J = np.zeros((n, n), np.float32)
        J[lo, hi] = rng.randint(0, 2, lo.size).astype(np.float32) * 2 - 1
        J = J + J.T
        m = IsingModel(IsingModelConfig(n_spins=n, use_sparse=not dense))
        m.set_couplings_from_matrix(torch.from_numpy(J))
        m.set_external_fields(torch.zeros(n))
        m.set_spins(torch.from_numpy((rng.randint(0, 2, n) * 2 - 1).astype(np.float32)))
        models.append(m)
        sizes.append(n)
    return models, sizes


def mixed(sweeps=200, k=8):
    cfg = GPUAnnealerConfig(n_sweeps=sweeps, initial_temp=3.0, final_temp=0.1, random_seed=7)
    out = {"models": 64, "n_range": [1000, 6000], "mean_degree": 8, "replicas_per_model": k, "sweeps": sweeps}
    for path, dense in (("ragged", False), ("densified_by_size", True)):
        models, sizes = mixed_models(dense=dense)
        bp = BatchProcessor(cfg, BatchConfig(batch_size=64, replicas_per_model=k))
        bp.process_models_batch(models[:2])  # warm-up of the path (library load, code objects)
        torch.cuda.synchronize()
        t0 = time.time()
        res = bp.process_models_batch(models)
        out[path] = {"wall_s": time.time() - t0, "best_energy_sum": float(sum(r.best_energy for r in res))}
    out["speedup_ragged_over_densified"] = out["densified_by_size"]["wall_s"] / out["ragged"]["wall_s"]
    # the ragged kernel alone: one engine of the 64 models, the same replicas and sweeps at a fixed temperature ladder
    models, sizes = mixed_models()
    from spin_glass_anneal_rl_amd.ising_model import coo_to_csr
    probs = [coo_to_csr(m.couplings) + (np.zeros(m.n_spins, np.float32),) for m in models]
    with sg.AnnealEngine(0) as e:
        e.set_csr_batch(probs)
        e.init_replicas(64 * k, seed=3)
        e.set_temperatures(np.tile(ladder(k), 64))
        ms, launches = timed_sweeps(e, sweeps)
        attempts = k * sum(sizes) * sweeps
        out["ragged_kernel"] = {"attempts_per_s": attempts / (ms * 1e-3), "kernel_ms": ms, "launches": launches,
                                "imbalance_bound_mean_over_max_n": float(np.mean(sizes) / np.max(sizes)),
                                "kernel": e.last_kernel(), "describe": e.describe()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["overhead", "copies", "mixed"])
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    parts = {"overhead": overhead, "copies": copies, "mixed": mixed}
    report = {"device": torch.cuda.get_device_name(0), "timing": "sga_enable_timing (device events), warmed up"}
    for name, fn in parts.items():
        if args.only in (None, name):
            report[name] = fn()
            print(name, json.dumps(report[name], default=float)[:400], flush=True)
    if not args.no_write:
        with open(OUT, "w") as f:
            json.dump(report, f, indent=1, default=float)


if __name__ == "__main__":
    main()
