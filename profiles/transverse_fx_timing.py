"""Simulated quantum annealing on dense couplings with real-valued J (sga_sweep_transverse_dense under option
"clf_fixed_point", csrc/sweep_transverse_fx.hip): time of a transverse sweep carried by the fixed-point cached fields
against the forms it is built from and the routes it replaces, written to profiles/transverse_fx.json.

Two problems at n = 10^4, 32 instances x 32 slices = 1024 replicas, fp32 rows, int32 fields:
  quarter   bench.py's headline +-1 matrix (make_sk_instance) times 1/4, h = 0: k = 2; the schedule of DESIGN.md 4.11
            scaled with it -- every slice at P T = 30 / 4, Gamma = 30 / 4 ("mid") and 1 / 4 ("end")
  sk_grid   the binary-grid SK instance of DESIGN.md 4.1i (profiles/dense_fixed_point_timing.py: J = rint(1024 randn) /
            1024, h on the same grid): k = 10; P T = 30, Gamma = 30 and 1
Each point is reached by `--presweeps` (50) transverse sweeps at its Gamma from the seed's random spins.  Figures per
problem and point, median [min, max] ms of `--reps` (20) calls after `--warmup` (3), event time on torch's stream:
  transverse_fx_ms      one sweep_transverse_dense(1, P, k): two launches, each over half the slices; beside it
                        hottest_acceptance: the largest accepted share of any slice over the timed calls
  cached_sweep_ms       (a) one classical cached fixed-point sga_sweep of the same engine at the slice temperature, from the
                        same state: one launch over all slices
  row_sweep_ms          (b) one row-per-proposal sga_sweep (field cache off, option row_shared = 0) from the same state
  host_route_ms         (c) what a user did before, host clocked, median of 3: per half-sweep spins(), an h per slice
                        (h + k (s_up + s_dn) for the moving slices; a standing slice is given T = 0 and a field 10^6 s that no
                        proposal passes), set_dense_shared with one model per slice, init_replicas(s0 = the spins),
                        set_temperatures, sweep(1); twice for a sweep.  host_route_same_chain: its spins are the device step's
usage: transverse_fx_timing.py [--reps 20] [--warmup 3] [--presweeps 50] [--n 10000] [--problem quarter|sk_grid|both]
                               [--out FILE] [--no-write]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
OUT = os.path.join(ROOT, "profiles", "transverse_fx.json")
SEED = 42


def host_route_half(helper, J, h, S, T, P, k, parity, sweep):
    """One half-sweep through the public calls of an engine without the dense transverse step; returns the spins after it."""
    R, n = S.shape
    G = R // P
    cube = S.reshape(G, P, n).astype(np.float32)
    H = h[None, None, :] + np.float32(k) * (np.roll(cube, -1, axis=1) + np.roll(cube, 1, axis=1))  # (fp32: one rounding)
    standing = (np.arange(P) % 2) != parity
    H[:, standing, :] = 1.0e6 * cube[:, standing, :]
    temps = np.where(np.tile(standing, G), 0.0, T)
    helper.set_dense_shared(J, H.reshape(R, n))
    helper.init_replicas(R, seed=SEED, s0=S)
    helper.set_temperatures(temps)
    helper.set_counters(sweep, 0)  # the sweep's own Philox coordinates
    helper.sweep(1)
    return helper.spins()


def measure(J, h, T, gamma, G, P, a):
    import torch
    import spin_glass_anneal_rl_amd as sg
    from cluster_moves_timing import event_ms
    n, R = J.shape[0], G * P
    k = sg.transverse_coupling(gamma, T / P, P)
    res = {"n": n, "instances": G, "slices": P, "replicas": R, "slice_temperature": T, "gamma": gamma, "k_perp": k,
           "warmup": a.warmup, "reps": a.reps, "presweeps": a.presweeps}
    stream = torch.cuda.current_stream().cuda_stream
    with sg.AnnealEngine(0) as e:
        e.use_stream(stream)
        e.set_option("clf_fixed_point", 1)
        e.set_field_cache("on")
        e.set_dense(J, h)
        e.init_replicas(R, seed=SEED)
        e.set_temperatures(T)
        e.sweep_transverse_dense(a.presweeps, P, k)
        S0, counters = e.spins(), e.counters()
        acc0 = e.stats()[0]
        res["transverse_fx_ms"] = event_ms(torch, lambda: e.sweep_transverse_dense(1, P, k), a.warmup, a.reps)
        res["hottest_acceptance"] = float((e.stats()[0] - acc0).max()) / float((a.warmup + a.reps) * n)
        res["transverse_fx_kernel"] = e.last_kernel()
        res["describe"] = e.describe()
        # (a) the classical cached fixed-point sweep, from the state the presweeps left
        e.init_replicas(R, seed=SEED, s0=S0)
        e.set_temperatures(T)
        e.set_counters(*counters)
        acc0 = e.stats()[0]
        res["cached_sweep_ms"] = event_ms(torch, lambda: e.sweep(1), a.warmup, a.reps)
        res["cached_sweep_hottest_acceptance"] = float((e.stats()[0] - acc0).max()) / float((a.warmup + a.reps) * n)
        res["cached_sweep_kernel"] = e.last_kernel()
        # the device step once more from S0, for the host route to be held against
        e.init_replicas(R, seed=SEED, s0=S0)
        e.set_temperatures(T)
        e.set_counters(*counters)
        e.sweep_transverse_dense(1, P, k)
        want = e.spins()
    with sg.AnnealEngine(0) as rows:  # (b) a row per proposal
        rows.use_stream(stream)
        rows.set_option("row_shared", 0)
        rows.set_field_cache("off")
        rows.set_dense(J, h)
        rows.init_replicas(R, seed=SEED, s0=S0)
        rows.set_temperatures(T)
        rows.set_counters(*counters)
        res["row_sweep_ms"] = event_ms(torch, lambda: rows.sweep(1), a.warmup, a.reps)
        res["row_sweep_kernel"] = rows.last_kernel()
    try:  # (c) the host route, and that it walks the same chain as the device step
        h_host = h.cpu().numpy().astype(np.float32)
        with sg.AnnealEngine(0) as helper:
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                S = S0
                for parity in (0, 1):
                    S = host_route_half(helper, J, h_host, S, T, P, k, parity, counters[0])
                times.append((time.perf_counter() - t0) * 1e3)
            res["host_route_ms"] = [float(np.median(times)), float(min(times)), float(max(times))]
            res["host_route_same_chain"] = bool(np.array_equal(S, want))
    except sg.SpinGlassError as exc:  # (recorded, not hidden: the figure is then missing)
        res["host_route_error"] = str(exc)
    res["transverse_fx_over_cached_sweep"] = res["transverse_fx_ms"][0] / res["cached_sweep_ms"][0]
    res["row_sweep_over_transverse_fx"] = res["row_sweep_ms"][0] / res["transverse_fx_ms"][0]
    if "host_route_ms" in res:
        res["host_route_over_transverse_fx"] = res["host_route_ms"][0] / res["transverse_fx_ms"][0]
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--presweeps", type=int, default=50)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--instances", type=int, default=32)
    ap.add_argument("--slices", type=int, default=32)
    ap.add_argument("--problem", default="both", choices=["quarter", "sk_grid", "both"])
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    torch.cuda.set_stream(torch.cuda.Stream())  # (a stream of its own: handle 0 would mean the engine's own)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    for name in (["quarter", "sk_grid"] if a.problem == "both" else [a.problem]):
        if name == "quarter":
            import bench
            J = bench.make_sk_instance(a.n, 2, torch.device("cuda", 0)).float() * 0.25  # (the headline workload's matrix: seed 2)
            h = torch.zeros(a.n, dtype=torch.float32, device=J.device)
            T, gammas = 7.5, (7.5, 0.25)
        else:
            g = torch.Generator("cuda").manual_seed(3)
            J = torch.triu(torch.round(torch.randn((a.n, a.n), device="cuda", generator=g) * 1024.0) / 1024.0, 1)
            h = torch.round(torch.randn(a.n, device="cuda", generator=g) * 1024.0) / 1024.0
            J = J + J.T
            T, gammas = 30.0, (30.0, 1.0)
        for point, gamma in zip(("mid", "end"), gammas):
            key = "%s_T%g_%s" % (name, T, point)
            got = measure(J, h, T, gamma, a.instances, a.slices, a)
            print(json.dumps({key: got}, indent=1), flush=True)
            doc[key] = got
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
