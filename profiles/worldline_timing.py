"""World-line cluster updates (sga_worldline_clusters, csrc/worldline_clusters.hip): time of one cluster sweep beside one
transverse sweep of the same engine and beside the host route it replaces, written to profiles/worldline.json (DESIGN.md
"World-line clusters").

Two shapes, each one engine on torch's stream so that torch events bracket its work:
  lattice_22   a 3-D +-J lattice of 22^3 = 10 648 spins with periodic boundaries, 32 instances x 32 slices (32-bit words)
  c3           bench.py's C3 graph (n = 10^4, degree ~32), 16 instances x 64 slices (64-bit words)
Every slice runs at P T with T = 0.05.  Per Gamma in (1, 0.05): a fresh set of replicas, `--presweeps` (50) transverse sweeps
at that Gamma, then median [min, max] ms of `--reps` (20) calls after `--warmup` (3), event time:
  clusters_ms      one worldline_clusters(1, P, p_bond) at p_bond = bond_probability(k_perp, P T)
  clusters_8_ms    one call of 8 sweeps, per sweep (one launch; the transposes in and out spread over 8)
  transverse_ms    one sweep_transverse(1, P, k_perp) in the same session
and from the counts of the timed calls: the mean segment length (P n / segments formed per sweep) and the flipped share
(slice spins flipped / (P n) per sweep), and the acceptance of the transverse sweeps.
  host_route_ms    what a user did before, host clocked, once: spins(), the reference's step vectorised in numpy (Philox
                   and all; np.exp in fp32 stands in for the engine's exp, so a uniform that falls between the two values
                   of one exp takes the chain elsewhere: the count of differing spins is recorded, not asserted), set_spins()
`--anneal SWEEPS`: the residual energy of SimulatedQuantumAnnealing.run on the lattice, 32 slices x 4 instances, Gamma 3 ->
0.01 linearly, with and without the clusters at equal transverse sweeps over the same `--seeds` (4) seeds: the best energy
per site of each run.
`--ab LABEL`: clusters_ms, clusters_8_ms and transverse_ms per Gamma alone (no host route), of the library in use
(SGA_LIBRARY_PATH), appended as one round under doc["ab_rounds"][LABEL][shape] (profiles/ab_rounds.py); nothing else of the
file changes.
usage: worldline_timing.py [--reps 20] [--warmup 3] [--presweeps 50] [--shape lattice_22|c3|both] [--anneal 0] [--seeds 4]
                           [--no-host-route] [--ab LABEL] [--out FILE] [--no-write]"""
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
OUT = os.path.join(ROOT, "profiles", "worldline.json")
T_QUANTUM, GAMMAS, SEED = 0.05, (1.0, 0.05), 42
M32 = np.uint64(0xFFFFFFFF)


def philox_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit words; returns words 0 and 1."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1


def host_sweep(graph, h, S, T, P, p_bond, seed, rnd):
    """One cluster sweep of tests/worldline_reference.py, all groups at once in numpy; in place on S [R, n] int8."""
    rowptr, col, val = graph
    R, n = S.shape
    G = R // P
    cube = S.reshape(G, P, n)
    thr = np.uint64(int(np.floor(p_bond * 16777216.0)))
    q = np.arange(R, dtype=np.uint64).reshape(G, P)
    lanes = np.arange(P)[None, :]
    gidx = np.arange(G)[:, None]
    vi = val.astype(np.int64)
    for i in range(n):
        lo, hi = rowptr[i], rowptr[i + 1]
        dots = (cube[:, :, col[lo:hi]].astype(np.int64) * vi[lo:hi]).sum(axis=2)
        w0, w1 = philox_np(np.full((G, P), i, np.uint64), np.uint64(rnd), q, np.uint64(4), seed & 0xFFFFFFFF, seed >> 32)
        column = cube[:, :, i]
        bond = (column == np.roll(column, -1, axis=1)) & ((w0 >> np.uint64(8)) < thr)
        heads = ~np.roll(bond, 1, axis=1)
        heads[~heads.any(axis=1), 0] = True
        f = np.maximum.accumulate(np.where(heads, lanes, -1), axis=1)
        f = np.where(f < 0, f.max(axis=1, keepdims=True), f)  # the wrap through slice 0
        flat = (gidx * P + f).ravel()
        A = np.bincount(flat, weights=dots.ravel(), minlength=R).reshape(G, P)
        m = np.bincount(flat, minlength=R).reshape(G, P)
        dE = 2.0 * column * (A + m * np.float64(h[i]))
        u = (w1 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
        with np.errstate(over="ignore"):
            flip = heads & ((dE <= 0.0) | (u < np.exp((-dE / T).astype(np.float32))))
        column[np.take_along_axis(flip, f, axis=1)] *= -1


def measure(name, graph, G, P, a):
    import torch
    import spin_glass_anneal_rl_amd as sg
    from cluster_moves_timing import event_ms
    n, R = len(graph[0]) - 1, G * P
    h = np.zeros(n, np.float32)
    T = P * T_QUANTUM
    res = {"n": n, "instances": G, "slices": P, "replicas": R, "slice_temperature": T, "warmup": a.warmup, "reps": a.reps,
           "presweeps": a.presweeps, "entries": int(len(graph[1]))}
    with sg.AnnealEngine(0) as e:
        e.use_stream(torch.cuda.current_stream().cuda_stream)
        e.set_csr(*graph, h)
        for gamma in GAMMAS:
            k = sg.transverse_coupling(gamma, T_QUANTUM, P)
            pb = sg.bond_probability(k, T)
            e.init_replicas(R, seed=SEED)
            e.set_temperatures(T)
            e.sweep_transverse(a.presweeps, P, k)
            out = {"gamma": gamma, "k_perp": k, "p_bond": pb}
            out["transverse_ms"] = event_ms(torch, lambda: e.sweep_transverse(1, P, k), a.warmup, a.reps)
            acc0, att0 = (x.sum() for x in e.stats())
            e.sweep_transverse(4, P, k)
            acc1, att1 = (x.sum() for x in e.stats())
            out["transverse_acceptance"] = float(acc1 - acc0) / float(att1 - att0)
            out["clusters_ms"] = event_ms(torch, lambda: e.worldline_clusters(1, P, pb), a.warmup, a.reps)
            out["clusters_kernel"] = e.last_kernel()
            out["clusters_8_ms"] = [t / 8 for t in event_ms(torch, lambda: e.worldline_clusters(8, P, pb), a.warmup, a.reps)]
            st = e.worldline_clusters(4, P, pb, stats=True).sum(axis=0)
            out["mean_segment_length"] = 4.0 * R * n / float(st[0])
            out["segments_flipped_share"] = float(st[1]) / float(st[0])
            out["spins_flipped_share"] = float(st[2]) / (4.0 * R * n)
            out["clusters_over_transverse"] = out["clusters_ms"][0] / out["transverse_ms"][0]
            if not a.no_host_route and not a.ab:
                rnd = 1000
                S0 = e.spins()
                e.worldline_clusters(1, P, pb, round=rnd)
                want = e.spins()
                t0 = time.perf_counter()
                S = e.spins()
                t1 = time.perf_counter()
                S[:] = S0
                host_sweep(graph, h, S, T, P, pb, SEED, rnd)
                t2 = time.perf_counter()
                for r in range(R):
                    e.set_spins(r, S[r])
                t3 = time.perf_counter()
                out["host_route_ms"] = (t3 - t0) * 1e3
                out["host_route_parts_ms"] = {"spins": (t1 - t0) * 1e3, "numpy_sweep": (t2 - t1) * 1e3, "set_spins": (t3 - t2) * 1e3}
                out["host_route_spins_differing"] = int(np.count_nonzero(S != want))
                out["host_route_over_clusters"] = out["host_route_ms"] / out["clusters_ms"][0]
            res["gamma_%g" % gamma] = out
        res["library"] = os.path.basename(sg._native.library_path())
    return res


def anneal(graph, a):
    import torch
    import spin_glass_anneal_rl_amd as sg
    n = len(graph[0]) - 1

    class Model:  # (what run() reads of a model, without a dense n x n matrix on the way)
        n_spins, device = n, torch.device("cuda", 0)

        def load_into(self, eng):
            eng.set_csr(*graph, np.zeros(n, np.float32))

    model = Model()
    out = {"n": n, "slices": 32, "instances": 4, "temperature": T_QUANTUM, "sweeps": a.anneal, "gamma": [3.0, 0.01], "runs": []}
    for seed in range(1, a.seeds + 1):
        row = {"seed": seed}
        for key, on in (("transverse_only", False), ("with_clusters", True)):
            cfg = sg.SimulatedQuantumAnnealingConfig(n_slices=32, n_instances=4, temperature=T_QUANTUM, n_sweeps=a.anneal, seed=seed,
                                                     transverse_field=sg.TransverseField("linear_decrease", 3.0, 0.01),
                                                     measure_interval=max(a.anneal // 10, 1), worldline_clusters=on, device_index=0)
            sqa = sg.SimulatedQuantumAnnealing(cfg)
            t0 = time.perf_counter()
            r = sqa.run(model)
            row[key] = {"best_energy_per_site": r.best_energy / n, "seconds": time.perf_counter() - t0,
                        "distinct_final_energies": int(len(np.unique(sqa.final_energies)))}
        out["runs"].append(row)
    for key in ("transverse_only", "with_clusters"):
        out["mean_" + key] = float(np.mean([r[key]["best_energy_per_site"] for r in out["runs"]]))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--presweeps", type=int, default=50)
    ap.add_argument("--shape", default="both", choices=["lattice_22", "c3", "both"])
    ap.add_argument("--anneal", type=int, default=0)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--no-host-route", action="store_true")
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
    from cluster_moves_timing import lattice
    shapes = {}
    if a.shape in ("lattice_22", "both"):
        shapes["lattice_22"] = (lattice(22, 1), 32, 32)
    if a.shape in ("c3", "both"):
        import bench
        shapes["c3"] = (bench.make_sparse_instance(10000, 16, 3), 16, 64)
    for name, (graph, G, P) in shapes.items():
        got = measure(name, graph, G, P, a)
        if a.ab:
            import ab_rounds
            figures = {"gamma_%g_%s" % (gamma, key): got["gamma_%g" % gamma][key] for gamma in GAMMAS
                       for key in ("clusters_ms", "clusters_8_ms", "transverse_ms")}
            ab_rounds.append(doc, a.ab, name, figures, got["library"])
        else:
            del got["library"]
            doc[name] = got
    if a.anneal > 0:
        doc["residual_energy_lattice_22"] = anneal(lattice(22, 1), a)
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
