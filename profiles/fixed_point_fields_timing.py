"""Cached local fields over real-valued CSR couplings (engine option "clf_fixed_point", csrc/sweep_clf_csr.hip): the
fixed-point form against the streaming row-per-proposal form on the same chain, written to
profiles/fixed_point_fields.json.  Kernel times come from the engine's own event timing (sga_enable_timing); wall
times bracket the same calls.  Kernel statistics come from a separate run of this script under
`rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/fixed_point_fields_timing.py --quick --no-write`
(the top rows of its top_kernels table: profiles/fixed_point_fields_kernel_stats.csv, durations in ns).

  c5     BASELINE configs[4] at 100 cities (10^4 spins, int64 fields), 2048 replicas on 32 ladders of 64 temperatures
         200 -> 2, an exchange round every 10 sweeps -- bench.py's cached_csr_variant cadence: sweeps 20..30, and
         sweeps 200..210 (after cooling)
  int32  a binary-grid instance (couplings rint(randn * 1024) / 1024, mean degree 16, 20 000 spins, int32 fields),
         1024 replicas on a 10 -> 0.1 ladder: sweeps 20..30 and 100..110

Each line: value (attempts/s), acceptance, ms per sweep (wall and kernel) and the instantiation -- reported beside the
graded figure of bench.py (one row per proposal), never instead of it.
usage: fixed_point_fields_timing.py [--quick] [--no-write]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spin_glass_anneal_rl_amd as sg  # noqa: E402
from spin_glass_anneal_rl_amd import encoders as enc  # noqa: E402
from spin_glass_anneal_rl_amd.sharded import ShardedTempering  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixed_point_fields.json")


def ladder(R, tmax, tmin):
    return np.asarray([tmax * (tmin / tmax) ** (i / max(R - 1, 1)) for i in range(R)])


def c5_problem():
    rs = np.random.RandomState(5)  # bench.py's C5 point set
    xy = rs.rand(100, 2) * 100.0
    d = np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1])
    rp, ci, v, h = enc.tsp_csr(d, city_visit=200.0, position_fill=200.0, device="cuda")[:4]
    return (rp, ci, v, h), 100 * 100


def grid_problem(n=20000, deg=16, seed=3):
    rng = np.random.RandomState(seed)
    i = rng.randint(0, n, n * deg // 2)
    j = rng.randint(0, n, i.size)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    key = np.unique(lo.astype(np.int64)[lo != hi] * n + hi[lo != hi])  # distinct pairs i < j
    lo, hi = key // n, key % n
    w = np.rint(rng.randn(key.size) * 1024.0) / 1024.0
    w[w == 0.0] = 1.0 / 1024.0
    rows, cols = np.concatenate([lo, hi]), np.concatenate([hi, lo])
    vals = np.concatenate([w, w]).astype(np.float32)
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    h = (rng.randn(n) * 0.5).astype(np.float32)
    return (rp, cols[order].astype(np.int32), vals[order], h), n


def measure(problem, n, R, temps, n_ladders, windows, fixed_point, exchange_interval=10):
    """{window: line} for sweeps [a, b) of each window, the run driven as bench.py drives it."""
    csr, lines = problem, {}
    with sg.AnnealEngine(0) as e:
        if fixed_point:
            e.set_option("clf_fixed_point", 1)
        e.set_field_cache("on" if fixed_point else "off")
        e.set_csr(*csr)
        pt = ShardedTempering(e, R_local=R, rank=0, world=1, seed=42, slot_temps=temps, n_ladders=n_ladders, dist=None,
                              device=torch.device("cuda", 0))
        done = 0

        def run(k):
            nonlocal done
            while k > 0:
                chunk = min(k, exchange_interval - done % exchange_interval)
                pt.sweep(chunk)
                done += chunk
                k -= chunk
                if done % exchange_interval == 0:
                    pt.exchange(count=False)

        for a, b in windows:
            run(a - done)
            torch.cuda.synchronize()
            acc0 = int(e.stats()[0].sum())
            e.enable_timing(True)
            e.kernel_time(reset=True)
            t1 = time.perf_counter()
            run(b - a)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t1
            _, ms = e.kernel_time(reset=True)
            e.enable_timing(False)
            rate = (int(e.stats()[0].sum()) - acc0) / (float(R) * n * (b - a))
            deg = float(len(csr[1])) / n
            lines[f"{a}..{b}"] = {
                "value": float(R) * n * (b - a) / dt, "unit": "attempts/s", "acceptance_rate": rate,
                "ms_per_sweep": dt / (b - a) * 1e3, "kernel_ms_per_sweep": ms / (b - a),
                "kernel_instantiation": e.last_kernel(), "geometry": e.describe(),
                "byte_model": ("B = acceptance x (deg x 8 + 8) bytes per attempt" if fixed_point
                               else "one row per proposal: deg x 8 + 8 bytes per attempt"),
                "algorithmic_bytes_per_attempt": (rate if fixed_point else 1.0) * (deg * 8.0 + 8.0),
            }
        lines["energies_checksum"] = float(np.sum(e.energies()))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="the first window of each instance only")
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "note": "variant with its own byte model, beside the graded figure"}
    c5, n5 = c5_problem()
    w5 = [(20, 30)] if a.quick else [(20, 30), (200, 210)]
    t5 = np.tile(ladder(64, 200.0, 2.0), 32)
    res = {"cached_fixed_point": measure(c5, n5, 2048, t5, 32, w5, True),
           "streaming": measure(c5, n5, 2048, t5, 32, w5, False)}
    assert res["cached_fixed_point"]["energies_checksum"] == res["streaming"]["energies_checksum"], "chains differ"
    out["c5_100_cities"] = res
    del c5
    torch.cuda.empty_cache()
    g, ng = grid_problem()
    wg = [(20, 30)] if a.quick else [(20, 30), (100, 110)]
    tg = ladder(1024, 10.0, 0.1)
    res = {"cached_fixed_point": measure(g, ng, 1024, tg, 1, wg, True), "streaming": measure(g, ng, 1024, tg, 1, wg, False)}
    assert res["cached_fixed_point"]["energies_checksum"] == res["streaming"]["energies_checksum"], "chains differ"
    out["int32_binary_grid_20000"] = res
    print(json.dumps(out, indent=1))
    if not a.no_write:
        with open(OUT, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
