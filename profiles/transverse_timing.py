"""Simulated quantum annealing (sga_sweep_transverse, csrc/sweep_transverse.hip): time of a transverse sweep against the
plain sweeps of the same engine and against the host route it replaces, written to profiles/transverse.json (DESIGN.md
"Simulated quantum annealing").

Two shapes, each one engine on torch's stream so that torch events bracket its work:
  lattice_22   a 3-D +-J lattice of 22^3 = 10 648 spins with periodic boundaries, 32 instances x 32 slices
  c3           bench.py's C3 graph (n = 10^4, degree ~32), 16 instances x 64 slices
Every slice runs at P T with T = 0.05; `--presweeps` (50) transverse sweeps at Gamma = 1 go before anything is timed.
Figures per shape, median [min, max] ms of `--reps` (20) calls after `--warmup` (3), event time:
  transverse_ms        one sweep_transverse(1, P, k): two launches, each over half the slices
  transverse_8_ms      one call of 8 sweeps, per sweep (the staging of k_perp and the call's host part spread over 16 launches)
  sweep_one_update_ms  one sga_sweep of the same engine object set up again with option csr_updates_per_step = 0 (the narrow
                       one-update form the transverse kernel is modelled on), same problem, seed and replicas
  sweep_default_ms     ... in the default form (the option back at -1)
  sweep_one_update_rule_ms  the one-update form again with h_i = 2^-20 instead of 0: the dynamics are the same to within that
                       field, but h is no multiple of 1/2, so the problem's class has no accept table and every uphill proposal
                       evaluates the rule (an fp64 divide and the fp32 exp) -- as every proposal of a transverse sweep does, whose
                       h_eff is no integer
  host_route_ms        what a user did before, host clocked, median of 3: per half-sweep spins(), an h per slice
                       (h + k (s_up + s_dn) for the moving slices; a standing slice is given T = 0 and a field 10^6 s that no
                       proposal passes), set_csr_shared with one model per slice, init_replicas(s0 = the spins), set_temperatures,
                       sweep(1); twice for a sweep
doc[shape]["variants"] holds the figures of a build that is no longer there (h_eff from a pre-kernel: DESIGN.md 4.9); it is
carried over as it stands.
`--ab LABEL`: transverse_ms and transverse_8_ms alone, of the library in use (SGA_LIBRARY_PATH), appended as one round under
doc["ab_rounds"][LABEL][shape] (profiles/ab_rounds.py); nothing else of the file changes.
usage: transverse_timing.py [--reps 20] [--warmup 3] [--presweeps 50] [--shape lattice_22|c3|both] [--ab LABEL] [--out FILE] [--no-write]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
OUT = os.path.join(ROOT, "profiles", "transverse.json")
T_QUANTUM, GAMMA, SEED = 0.05, 1.0, 42


def host_route_half(sg, helper, graph, h, S, T, P, k, parity, sweep):
    """One half-sweep through the public calls of an engine that has no transverse step; returns the spins after it."""
    R, n = S.shape
    G = R // P
    cube = S.reshape(G, P, n).astype(np.float32)
    H = np.broadcast_to(h, (G, P, n)) + np.float32(k) * (np.roll(cube, -1, axis=1) + np.roll(cube, 1, axis=1))
    standing = (np.arange(P) % 2) != parity
    H[:, standing, :] = 1.0e6 * cube[:, standing, :]
    temps = np.where(np.tile(standing, G), 0.0, T)
    helper.set_csr_shared(graph[0], graph[1], graph[2], H.reshape(R, n))
    helper.init_replicas(R, seed=SEED, s0=S)
    helper.set_temperatures(temps)
    helper.set_counters(sweep, 0)  # the sweep's own Philox coordinates
    helper.sweep(1)
    return helper.spins()


def measure(name, graph, G, P, a):
    import torch
    import spin_glass_anneal_rl_amd as sg
    from cluster_moves_timing import event_ms
    n, R = len(graph[0]) - 1, G * P
    h = np.zeros(n, np.float32)
    T = P * T_QUANTUM
    k = sg.transverse_coupling(GAMMA, T_QUANTUM, P)
    res = {"n": n, "instances": G, "slices": P, "replicas": R, "slice_temperature": T, "gamma": GAMMA, "k_perp": k,
           "warmup": a.warmup, "reps": a.reps, "presweeps": a.presweeps, "entries": int(len(graph[1]))}

    def setup(e, updates_per_step, field=h):
        e.set_option("csr_updates_per_step", updates_per_step)
        e.set_csr(*graph, field)
        e.init_replicas(R, seed=SEED)
        e.set_temperatures(T)
        e.sweep_transverse(a.presweeps, P, k)

    with sg.AnnealEngine(0) as e:
        e.use_stream(torch.cuda.current_stream().cuda_stream)
        setup(e, -1)
        out = {"transverse_ms": event_ms(torch, lambda: e.sweep_transverse(1, P, k), a.warmup, a.reps),
               "transverse_8_ms": [t / 8 for t in event_ms(torch, lambda: e.sweep_transverse(8, P, k), a.warmup, a.reps)],
               "transverse_kernel": e.last_kernel()}
        if a.ab:
            return {"figures": {key: out[key] for key in ("transverse_ms", "transverse_8_ms")},
                    "library": os.path.basename(sg._native.library_path())}
        res.update(out)
        res["describe"] = e.describe()
        res["sweep_default_ms"] = event_ms(torch, lambda: e.sweep(1), a.warmup, a.reps)
        res["sweep_default_kernel"] = e.last_kernel()
        setup(e, 0)
        res["sweep_one_update_ms"] = event_ms(torch, lambda: e.sweep(1), a.warmup, a.reps)
        res["sweep_one_update_kernel"] = e.last_kernel()
        acc, att = e.stats()
        res["acceptance"] = float(acc.sum()) / float(att.sum())
        setup(e, 0, np.full(n, 2.0 ** -20, np.float32))
        res["sweep_one_update_rule_ms"] = event_ms(torch, lambda: e.sweep(1), a.warmup, a.reps)
        res["sweep_one_update_rule_kernel"] = e.last_kernel()
        setup(e, 0)
        # the host route, and that it walks the same chain as the device step (the fields of the standing slices freeze them)
        S0, counters = e.spins(), e.counters()
        e.sweep_transverse(1, P, k)
        want = e.spins()
        try:
            with sg.AnnealEngine(0) as helper:
                times = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    S = S0
                    for parity in (0, 1):
                        S = host_route_half(sg, helper, graph, h, S, T, P, k, parity, counters[0])
                    times.append((time.perf_counter() - t0) * 1e3)
                res["host_route_ms"] = [float(np.median(times)), float(min(times)), float(max(times))]
                res["host_route_same_chain"] = bool(np.array_equal(S, want))
        except sg.SpinGlassError as exc:  # (recorded, not hidden: the figure is then missing)
            res["host_route_error"] = str(exc)
    res["transverse_over_one_update"] = res["transverse_ms"][0] / res["sweep_one_update_ms"][0]
    res["transverse_over_one_update_rule"] = res["transverse_ms"][0] / res["sweep_one_update_rule_ms"][0]
    res["transverse_over_default"] = res["transverse_ms"][0] / res["sweep_default_ms"][0]
    if "host_route_ms" in res:
        res["host_route_over_transverse"] = res["host_route_ms"][0] / res["transverse_ms"][0]
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--presweeps", type=int, default=50)
    ap.add_argument("--shape", default="both", choices=["lattice_22", "c3", "both"])
    ap.add_argument("--ab", default="", metavar="LABEL")
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
    shapes = {}
    if a.shape in ("lattice_22", "both"):
        from cluster_moves_timing import lattice
        shapes["lattice_22"] = (lattice(22, 1), 32, 32)
    if a.shape in ("c3", "both"):
        import bench
        shapes["c3"] = (bench.make_sparse_instance(10000, 16, 3), 16, 64)
    for name, (graph, G, P) in shapes.items():
        got = measure(name, graph, G, P, a)
        if a.ab:
            import ab_rounds
            ab_rounds.append(doc, a.ab, name, got["figures"], got["library"])
        else:
            got["variants"] = doc.get(name, {}).get("variants", {})
            doc[name] = got
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
