"""Cached local fields over real-valued DENSE couplings (engine option "clf_fixed_point", csrc/sweep_clf_fx.hip): the
fixed-point form against the row-per-proposal form (field cache off) on the same chain, and AUTO's per-replica routing,
written to profiles/dense_fixed_point.json.  Kernel times come from the engine's own event timing (sga_enable_timing);
wall times bracket the same calls.  Kernel statistics come from a separate run of this script under
`rocprofv3 --kernel-trace --stats -f csv -d <dir> -- python profiles/dense_fixed_point_timing.py --quick --no-write`
(the top rows of its top_kernels table: profiles/dense_fixed_point_kernel_stats.csv, durations in ns).

  physical  100 x 100 assignment in the physical convention (encoders.assignment_ising, weight 5: J = -2.5, integer
            costs: half-valued h), to_model(sparse=False): 10^4 spins, k = 1, int32 fields
  sk_grid   binary-grid SK: n = 10^4, J = rint(randn 1024) / 1024, h on the same grid: k = 10, int32 fields

1024 replicas on a 10 -> 0.1 ladder, sweeps 5..25 and 100..110; and sk_grid on a ladder that stays hot (1000 -> 20,
sweeps 5..10), to find where the row kernels win: AUTO's break-even (sga_route.cpp) is set from these lines.  Each line:
value (attempts/s), acceptance (all replicas, and the hottest one), ms per sweep (wall and kernel) and the instantiation
-- reported beside the graded figure of bench.py (one row per proposal), never instead of it.
usage: dense_fixed_point_timing.py [--quick] [--no-write]"""
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

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dense_fixed_point.json")


def ladder(R, tmax, tmin):
    return np.asarray([tmax * (tmin / tmax) ** (i / max(R - 1, 1)) for i in range(R)])


def physical_problem():
    rng = np.random.RandomState(1)
    b = enc.assignment_ising(100, 100, weight=5.0, costs=rng.randint(1, 10, 100 * 100).astype(np.float64))
    m = b.to_model(sparse=False)
    return m.couplings.float().cuda(), m.external_fields.float().cuda()


def sk_problem(n=10000, seed=3):
    g = torch.Generator("cuda").manual_seed(seed)
    J = torch.triu(torch.round(torch.randn((n, n), device="cuda", generator=g) * 1024.0) / 1024.0, 1)
    h = torch.round(torch.randn(n, device="cuda", generator=g) * 1024.0) / 1024.0
    return J + J.T, h


def measure(J, h, R, temps, windows, mode):
    """{window: line} for sweeps [a, b) of each window; mode = "fixed_point" | "rows" | "auto"."""
    n, lines = J.shape[0], {}
    with sg.AnnealEngine(0) as e:
        if mode != "rows":
            e.set_option("clf_fixed_point", 1)
        e.set_field_cache({"fixed_point": "on", "rows": "off", "auto": "auto"}[mode])
        e.set_dense(J, h)
        e.init_replicas(R, seed=42)
        e.set_ladder(temps)
        done = 0
        for a, b in windows:
            if a > done:
                e.sweep(a - done)
            torch.cuda.synchronize()
            acc0 = e.stats()[0].copy()
            e.enable_timing(True)
            e.kernel_time(reset=True)
            t1 = time.perf_counter()
            e.sweep(b - a)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t1
            _, ms = e.kernel_time(reset=True)
            e.enable_timing(False)
            done = b
            d_acc = (e.stats()[0] - acc0).astype(np.float64)
            rate = float(d_acc.sum()) / (float(R) * n * (b - a))
            row = 4.0 * n
            lines[f"{a}..{b}"] = {
                "value": float(R) * n * (b - a) / dt, "unit": "attempts/s", "acceptance_rate": rate,
                "hottest_replica_acceptance": float(d_acc.max()) / (n * (b - a)),
                "ms_per_sweep": dt / (b - a) * 1e3, "kernel_ms_per_sweep": ms / (b - a),
                "kernel_instantiation": e.last_kernel(), "geometry": e.describe(),
                "byte_model": ("one row per proposal: 4 n bytes per attempt" if mode == "rows"
                               else "B = acceptance x 4 n bytes per attempt (cached replicas)"),
                "algorithmic_bytes_per_attempt": (1.0 if mode == "rows" else rate) * row,
            }
        lines["energies"] = e.energies().copy()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="the first window of each instance only")
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "note": "variant with its own byte model, beside the graded figure"}
    R = 1024
    temps = ladder(R, 10.0, 0.1)
    windows = [(5, 25)] if a.quick else [(5, 25), (100, 110)]
    for name, make in (("physical_assignment_100x100", physical_problem), ("sk_binary_grid_10000", sk_problem)):
        J, h = make()
        res = {mode: measure(J, h, R, temps, windows, mode) for mode in ("fixed_point", "rows", "auto")}
        e_fx, e_rows, e_auto = (res[m].pop("energies") for m in ("fixed_point", "rows", "auto"))
        assert np.array_equal(e_fx, e_rows) and np.array_equal(e_auto, e_rows), "chains differ"
        res["energies_equal"] = True
        res["energies_checksum"] = float(np.sum(e_rows))
        out[name] = res
        if name.startswith("sk") and not a.quick:  # the same couplings on a ladder that stays hot
            hot = {mode: measure(J, h, R, ladder(R, 1000.0, 20.0), [(5, 10)], mode) for mode in ("fixed_point", "rows")}
            assert np.array_equal(hot["fixed_point"].pop("energies"), hot["rows"].pop("energies")), "chains differ"
            out[name + "_hot_ladder_1000_20"] = hot
        del J, h
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))
    if not a.no_write:
        with open(OUT, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
