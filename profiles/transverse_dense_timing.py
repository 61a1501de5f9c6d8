"""Simulated quantum annealing on dense couplings (sga_sweep_transverse_dense, csrc/sweep_transverse_clf.hip): time of a
transverse sweep carried by the cached local fields against the forms it is built from and the routes it replaces,
written to profiles/transverse_dense.json.

The instance is bench.py's headline +-1 matrix (make_sk_instance, n = 10^4), 32 instances x 32 slices = 1024 replicas, as
int8 rows and as fp32 rows, every slice at `--slice-temperature` (P T).  Two points of a schedule, each reached by
`--presweeps` (50) transverse sweeps at its Gamma from the seed's random spins: "mid" and "end" (`--gammas`).  The keys of
the file are T<slice temperature>_<storage>_<point>; the committed table holds the runs at P T = 30 (Gamma 30 and 1) and
at P T = 80 (`--slice-temperature 80 --gammas 80 2.7`), the hotter schedule.  Figures per storage and point, median [min, max] ms of `--reps` (20) calls after `--warmup` (3), event time on torch's stream:
  transverse_dense_ms   one sweep_transverse_dense(1, P, k): two launches, each over half the slices; beside it
                        hottest_acceptance: the largest accepted share of any slice over the timed calls
  cached_sweep_ms       (a) one classical cached-field sga_sweep of the same engine at the slice temperature, from the same
                        state: one launch over all slices
  row_sweep_ms          (b) one row-per-proposal sga_sweep (field cache off, option row_shared = 0) from the same state: the
                        floor of a design that streams a row per proposal
  host_route_ms         (c) what a user did before, host clocked, median of 3: per half-sweep spins(), an h per slice
                        (h + k (s_up + s_dn) for the moving slices; a standing slice is given T = 0 and a field 10^6 s that no
                        proposal passes), set_dense_shared with one model per slice, init_replicas(s0 = the spins),
                        set_temperatures, sweep(1); twice for a sweep
`--clf-waves W` times the new sweep alone under option clf_waves = W (keys ..._wavesW): the waves per slice.
`--ab LABEL`: transverse_dense_ms alone, of the library in use (SGA_LIBRARY_PATH), appended as one round under
doc["ab_rounds"][LABEL][key] (profiles/ab_rounds.py); nothing else of the file changes.
usage: transverse_dense_timing.py [--reps 20] [--warmup 3] [--presweeps 50] [--n 10000] [--storage i8|f32|both]
                                  [--slice-temperature 30] [--gammas MID END] [--clf-waves W] [--ab LABEL] [--out FILE] [--no-write]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
OUT = os.path.join(ROOT, "profiles", "transverse_dense.json")
SEED = 42


def host_route_half(helper, J, S, T, P, k, parity, sweep):
    """One half-sweep through the public calls of an engine without the dense transverse step; returns the spins after it."""
    R, n = S.shape
    G = R // P
    cube = S.reshape(G, P, n).astype(np.float32)
    H = np.float32(k) * (np.roll(cube, -1, axis=1) + np.roll(cube, 1, axis=1))
    standing = (np.arange(P) % 2) != parity
    H[:, standing, :] = 1.0e6 * cube[:, standing, :]
    temps = np.where(np.tile(standing, G), 0.0, T)
    helper.set_dense_shared(J, H.reshape(R, n))
    helper.init_replicas(R, seed=SEED, s0=S)
    helper.set_temperatures(temps)
    helper.set_counters(sweep, 0)  # the sweep's own Philox coordinates
    helper.sweep(1)
    return helper.spins()


def measure(J, storage, point, gamma, G, P, a):
    import torch
    import spin_glass_anneal_rl_amd as sg
    from cluster_moves_timing import event_ms
    n, R, T = J.shape[0], G * P, float(a.slice_temperature)
    h = torch.zeros(n, dtype=torch.float32, device=J.device)
    k = sg.transverse_coupling(gamma, T / P, P)
    res = {"n": n, "instances": G, "slices": P, "replicas": R, "storage": storage, "slice_temperature": T, "gamma": gamma,
           "k_perp": k, "warmup": a.warmup, "reps": a.reps, "presweeps": a.presweeps}
    stream = torch.cuda.current_stream().cuda_stream
    with sg.AnnealEngine(0) as e:
        e.use_stream(stream)
        if a.clf_waves:
            e.set_option("clf_waves", a.clf_waves)
        e.set_field_cache("on")
        e.set_dense(J, h, storage=storage)
        e.init_replicas(R, seed=SEED)
        e.set_temperatures(T)
        e.sweep_transverse_dense(a.presweeps, P, k)
        S0, counters = e.spins(), e.counters()
        acc0 = e.stats()[0]
        res["transverse_dense_ms"] = event_ms(torch, lambda: e.sweep_transverse_dense(1, P, k), a.warmup, a.reps)
        res["hottest_acceptance"] = float((e.stats()[0] - acc0).max()) / float((a.warmup + a.reps) * n)
        res["transverse_dense_kernel"] = e.last_kernel()
        if a.clf_waves or a.ab:  # (the waves per slice, a round of an A/B: the new sweep alone)
            res["library"] = os.path.basename(sg._native.library_path())
            return res
        res["describe"] = e.describe()
        # (a) the classical cached-field sweep, from the state the presweeps left
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
        rows.set_dense(J, h, storage=storage)
        rows.init_replicas(R, seed=SEED, s0=S0)
        rows.set_temperatures(T)
        rows.set_counters(*counters)
        res["row_sweep_ms"] = event_ms(torch, lambda: rows.sweep(1), a.warmup, a.reps)
        res["row_sweep_kernel"] = rows.last_kernel()
    try:  # (c) the host route, and that it walks the same chain as the device step
        with sg.AnnealEngine(0) as helper:
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                S = S0
                for parity in (0, 1):
                    S = host_route_half(helper, J, S, T, P, k, parity, counters[0])
                times.append((time.perf_counter() - t0) * 1e3)
            res["host_route_ms"] = [float(np.median(times)), float(min(times)), float(max(times))]
            res["host_route_same_chain"] = bool(np.array_equal(S, want))
    except sg.SpinGlassError as exc:  # (recorded, not hidden: the figure is then missing)
        res["host_route_error"] = str(exc)
    res["transverse_dense_over_cached_sweep"] = res["transverse_dense_ms"][0] / res["cached_sweep_ms"][0]
    res["row_sweep_over_transverse_dense"] = res["row_sweep_ms"][0] / res["transverse_dense_ms"][0]
    if "host_route_ms" in res:
        res["host_route_over_transverse_dense"] = res["host_route_ms"][0] / res["transverse_dense_ms"][0]
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--presweeps", type=int, default=50)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--instances", type=int, default=32)
    ap.add_argument("--slices", type=int, default=32)
    ap.add_argument("--slice-temperature", type=float, default=30.0)
    ap.add_argument("--gammas", type=float, nargs=2, default=[30.0, 1.0], metavar=("MID", "END"))
    ap.add_argument("--storage", default="both", choices=["i8", "f32", "both"])
    ap.add_argument("--clf-waves", type=int, default=0, help="option clf_waves: transverse_dense_ms alone, key suffix _wavesN")
    ap.add_argument("--ab", default="", metavar="LABEL")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    torch.cuda.set_stream(torch.cuda.Stream())  # (a stream of its own: handle 0 would mean the engine's own)
    import bench
    J = bench.make_sk_instance(a.n, 2, torch.device("cuda", 0))  # (the headline workload's matrix: seed 2)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    for storage in (["i8", "f32"] if a.storage == "both" else [a.storage]):
        for point, gamma in zip(("mid", "end"), a.gammas):
            key = "T%g_%s_%s" % (a.slice_temperature, storage, point)  # (runs at several slice temperatures share the file)
            if a.clf_waves:
                key += "_waves%d" % a.clf_waves
            got = measure(J, storage, point, gamma, a.instances, a.slices, a)
            print(json.dumps({key: got}, indent=1), flush=True)
            if a.ab:
                import ab_rounds
                ab_rounds.append(doc, a.ab, key, {"transverse_dense_ms": got["transverse_dense_ms"]}, got["library"])
            else:
                doc[key] = got
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
