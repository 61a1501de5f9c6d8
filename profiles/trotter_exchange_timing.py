"""Time links and the exchange between Trotter groups along the transverse field (sga_get_time_links,
sga_exchange_transverse, csrc/trotter_exchange.hip): the times of the two calls beside a transverse sweep and the host
route they replace, written to profiles/trotter_exchange.json.

Two shapes, 32 instances x 32 slices each, one engine on torch's stream so that torch events bracket its work:
  lattice_22   the 3-D +-J lattice of 22^3 = 10 648 spins of profiles/transverse_timing.py (CSR rows), T = 0.05, Gamma = 1
  dense_i8     bench.py's headline +-1 matrix (make_sk_instance, n = 10^4) as int8 rows with the field cache on, every
               slice at P T = 30, Gamma = 30
each after `--presweeps` (50) transverse sweeps under a k ladder (Gamma_g = Gamma 2^((g - 16) / 32)).  Figures are median
[min, max] ms of `--reps` (20) calls after `--warmup` (3), event time:
  time_links_device_ms       time_links(P, out=<int64 CUDA tensor>): the memset and the count kernel
  time_links_host_ms         time_links(P): the same and the copy of 32 counts
  count_gb_per_s             R sstride bytes over the median of time_links_device_ms; read_probe_gb_per_s beside it is
                             the streaming-read probe of bench.py --full (sga_probe_read_bandwidth, 4 GiB)
  exchange_ms                one exchange_transverse at the ladder (counts, decision, swap, bests, the copy of 2 x 32 values),
                             alternating parity; accepted_share of its pairs over the timed calls
  exchange_all_swap_ms       the same where every pair swaps (one k for all groups: x = 0)
  exchange_none_ms           the same where no pair is decided (every T infinite: the decision leaves, the swap's
                             workgroups return at the flag) -- the launches are not timed one by one from Python, so the parts
                             are differences: decide_and_bests_ms = exchange_none - time_links_host, swap_ms =
                             exchange_all_swap - exchange_none
  transverse_ms              one transverse sweep in the same state
  spins_ms                   spins() alone (host clock)
  host_route_ms              the route the call replaces, host clock, `--host-reps` (3): spins(), the counts and the decisions
                             in numpy, set_spins() per slice of the swapped groups; its parts beside it
dense_i8 only: sweep_after_exchange_ms, one dense transverse sweep directly after an exchange in which every pair swapped
(the field rows traded), and sweep_after_reseed_ms, the same sweep after set_spins of the same spins (the fields seeded
again): single calls, `--reps` times each.
`--physics SWEEPS` (0 = skip): SimulatedQuantumAnnealing.run on lattice_22 at constant Gamma = 1 (the path_integral_mc
setting), T = 0.05, 8 instances x 32 slices on the geometric ladder `--ladder LO HI` (0.5 2), with
field_exchange_interval 5 and without, `--seeds` (4) seeds: the acceptance per pair, the best energy per site of each run
(key physics_lattice_22_<LO>_<HI>).
`--ab LABEL`: time_links_device_ms, time_links_host_ms and exchange_ms alone, of the library in use (SGA_LIBRARY_PATH), appended as one round under
doc["ab_rounds"][LABEL][shape] (profiles/ab_rounds.py); nothing else of the file changes.
usage: trotter_exchange_timing.py [--reps 20] [--warmup 3] [--presweeps 50] [--host-reps 3] [--shape lattice_22|dense_i8|both]
                                  [--physics 0] [--ladder 0.5 2] [--seeds 4] [--out FILE] [--no-write]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
OUT = os.path.join(ROOT, "profiles", "trotter_exchange.json")
SEED, G, P = 42, 32, 32


def host_links(S, P):
    cube = S.reshape(-1, P, S.shape[1])
    return (cube != np.roll(cube, -1, axis=1)).sum(axis=(1, 2)).astype(np.int64)


def host_route(e, k, T, parity, rng):
    """spins(), counts and decisions in numpy, set_spins() per swapped slice: (total ms, parts, swapped pairs)."""
    t0 = time.perf_counter()
    S = e.spins()
    t1 = time.perf_counter()
    E = e.energies().reshape(-1, P).sum(axis=1)
    B = host_links(S, P)
    beta = 1.0 / T
    swaps = []
    for a in range(parity, len(B) - 1, 2):
        x = (beta[a] - beta[a + 1]) * (E[a] - E[a + 1]) + 2.0 * (beta[a] * k[a] - beta[a + 1] * k[a + 1]) * float(B[a] - B[a + 1])
        if rng.random_sample() < (1.0 if not x < 0.0 else np.exp(x)):
            swaps.append(a)
    t2 = time.perf_counter()
    for a in swaps:
        for p in range(P):
            e.set_spins(a * P + p, S[(a + 1) * P + p])
            e.set_spins((a + 1) * P + p, S[a * P + p])
    t3 = time.perf_counter()
    return (t3 - t0) * 1e3, {"spins_ms": (t1 - t0) * 1e3, "numpy_ms": (t2 - t1) * 1e3, "set_spins_ms": (t3 - t2) * 1e3}, len(swaps)


def stats(v):
    return [float(np.median(v)), float(min(v)), float(max(v))]


def measure(name, make_engine, sweep_name, slice_T, gamma, a):
    import torch
    import spin_glass_anneal_rl_amd as sg
    from cluster_moves_timing import event_ms
    R = G * P
    gam = gamma * 2.0 ** ((np.arange(G) - G // 2) / 32.0)
    k = np.asarray(sg.transverse_coupling(gam, slice_T / P, P), np.float32)
    res = {"instances": G, "slices": P, "replicas": R, "slice_temperature": slice_T, "gamma_ladder": [float(gam[0]), float(gam[-1])],
           "k_perp_ladder": [float(k[0]), float(k[-1])], "warmup": a.warmup, "reps": a.reps, "presweeps": a.presweeps}
    with make_engine(sg, torch) as e:
        sweep = getattr(e, sweep_name)
        e.set_temperatures(slice_T)
        sweep(a.presweeps, P, np.repeat(k[None, :], a.presweeps, axis=0))
        n, sstride = e.n, int(e.route_query().sstride)
        res["n"] = n
        out = torch.zeros(G, dtype=torch.int64, device="cuda")
        res["time_links_device_ms"] = event_ms(torch, lambda: e.time_links(P, out=out), a.warmup, a.reps)
        res["time_links_kernel"] = e.last_kernel()
        res["time_links_host_ms"] = event_ms(torch, lambda: e.time_links(P), a.warmup, a.reps)
        B = e.time_links(P)
        res["links_share"] = [float(B.min()) / (n * P), float(B.max()) / (n * P)]
        if a.ab:  # the count with its result on the device and on the host, and the exchange (results on the host)
            rnd = [1000]

            def exchange_round():
                rnd[0] += 1
                e.exchange_transverse(P, k, parity=rnd[0] & 1, round=rnd[0])
            figures = {key: res[key] for key in ("time_links_device_ms", "time_links_host_ms")}
            figures["exchange_ms"] = event_ms(torch, exchange_round, a.warmup, a.reps)
            return {"figures": figures, "library": os.path.basename(sg._native.library_path())}
        res["spin_bytes"] = R * sstride
        res["count_gb_per_s"] = R * sstride / (res["time_links_device_ms"][0] * 1e-3) / 1e9
        res["transverse_ms"] = event_ms(torch, lambda: sweep(1, P, k[None, :]), a.warmup, a.reps)
        rnd, taken = [1000], []

        def exchange(kk):
            rnd[0] += 1
            acc, _ = e.exchange_transverse(P, kk, parity=rnd[0] & 1, round=rnd[0])
            taken.append((int(acc.sum()) // 2, len(range(rnd[0] & 1, G - 1, 2))))
        res["exchange_ms"] = event_ms(torch, lambda: exchange(k), a.warmup, a.reps)
        res["exchange_kernel"] = e.last_kernel()
        res["accepted_share"] = float(sum(t[0] for t in taken[a.warmup:])) / float(sum(t[1] for t in taken[a.warmup:]))
        del taken[:]
        res["exchange_all_swap_ms"] = event_ms(torch, lambda: exchange(float(k[G // 2])), a.warmup, a.reps)
        assert all(t[0] == t[1] for t in taken)
        e.set_temperatures(np.inf)
        del taken[:]
        res["exchange_none_ms"] = event_ms(torch, lambda: exchange(k), a.warmup, a.reps)
        assert all(t[0] == 0 for t in taken)
        e.set_temperatures(slice_T)
        res["decide_and_bests_ms"] = res["exchange_none_ms"][0] - res["time_links_host_ms"][0]
        res["swap_ms"] = res["exchange_all_swap_ms"][0] - res["exchange_none_ms"][0]
        t = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            e.spins()
            t.append((time.perf_counter() - t0) * 1e3)
        res["spins_ms"] = stats(t)
        if sweep_name == "sweep_transverse_dense":
            one = lambda: event_ms(torch, lambda: sweep(1, P, k[None, :]), 0, 1)[0]  # noqa: E731
            after_x, after_s = [], []
            for _ in range(a.reps):
                exchange(float(k[G // 2]))
                after_x.append(one())
                e.set_spins(0, e.spins()[0])  # (the same spins: what moves is fields_valid)
                after_s.append(one())
            res["sweep_after_exchange_ms"], res["sweep_after_reseed_ms"] = stats(after_x), stats(after_s)
            res["fields_kept_valid_saves_ms"] = res["sweep_after_reseed_ms"][0] - res["sweep_after_exchange_ms"][0]
        rng = np.random.RandomState(SEED)
        T = np.full(G, slice_T)
        runs = [host_route(e, k.astype(np.float64), T, i & 1, rng) for i in range(a.host_reps)]
        res["host_route_ms"] = stats([r[0] for r in runs])
        res["host_route_parts_ms"] = {key: stats([r[1][key] for r in runs]) for key in runs[0][1]}
        res["host_route_swapped_pairs"] = [r[2] for r in runs]
        res["host_route_over_exchange"] = res["host_route_ms"][0] / res["exchange_ms"][0]
    return res


def physics(a):
    import torch
    import spin_glass_anneal_rl_amd as sg
    from cluster_moves_timing import lattice
    import scipy.sparse as sp
    g = lattice(22, 1)
    n = len(g[0]) - 1
    J = sp.csr_matrix((g[2], g[1], g[0]), shape=(n, n)).tocoo()
    model = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=True))
    model.couplings = torch.sparse_coo_tensor(torch.from_numpy(np.stack([J.row, J.col]).astype(np.int64)),
                                              torch.from_numpy(J.data.astype(np.float32)), (n, n)).coalesce()
    ladder = np.geomspace(a.ladder[0], a.ladder[1], 8)
    out = {"n": n, "instances": 8, "slices": 32, "temperature": 0.05, "gamma": 1.0, "field_ladder": ladder.tolist(), "sweeps": a.physics,
           "field_exchange_interval": 5, "seeds": [], "best_energy_per_site_with": [], "best_energy_per_site_without": [],
           "acceptance_per_pair": []}
    for seed in range(a.seeds):
        kw = dict(n_slices=32, n_instances=8, temperature=0.05, n_sweeps=a.physics, seed=100 + seed, measure_interval=50,
                  transverse_field=sg.TransverseField("constant", initial=1.0), field_ladder=ladder.tolist())
        on = sg.SimulatedQuantumAnnealing(sg.SimulatedQuantumAnnealingConfig(field_exchange_interval=5, **kw))
        off = sg.SimulatedQuantumAnnealing(sg.SimulatedQuantumAnnealingConfig(**kw))
        r_on, r_off = on.run(model), off.run(model)
        attempts, accepts = on.field_exchange_statistics
        out["seeds"].append(100 + seed)
        out["best_energy_per_site_with"].append(r_on.best_energy / n)
        out["best_energy_per_site_without"].append(r_off.best_energy / n)
        out["acceptance_per_pair"].append((accepts / np.maximum(attempts, 1)).tolist())
        out.setdefault("transverse_magnetization_with", []).append(on.transverse_magnetization.tolist())
    out["mean_acceptance_per_pair"] = np.mean(out["acceptance_per_pair"], axis=0).tolist()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--presweeps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--shape", default="both", choices=["lattice_22", "dense_i8", "both", "none"])
    ap.add_argument("--physics", type=int, default=0)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--ladder", type=float, nargs=2, default=[0.5, 2.0], metavar=("LO", "HI"))
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
    if not a.ab:
        from spin_glass_anneal_rl_amd.engine import probe_read_bandwidth
        doc["read_probe_gb_per_s"] = probe_read_bandwidth(0)

    def keep(shape, got):
        if a.ab:
            import ab_rounds
            ab_rounds.append(doc, a.ab, shape, got["figures"], got["library"])
        else:
            doc[shape] = got

    def lattice_engine(sg, torch):
        from cluster_moves_timing import lattice
        graph = lattice(22, 1)
        e = sg.AnnealEngine(0)
        e.use_stream(torch.cuda.current_stream().cuda_stream)
        e.set_csr(*graph, np.zeros(len(graph[0]) - 1, np.float32))
        e.init_replicas(G * P, seed=SEED)
        return e

    def dense_engine(sg, torch):
        import bench
        J = bench.make_sk_instance(10000, 2, torch.device("cuda", 0))
        e = sg.AnnealEngine(0)
        e.use_stream(torch.cuda.current_stream().cuda_stream)
        e.set_field_cache("on")
        e.set_dense(J, torch.zeros(J.shape[0], dtype=torch.float32, device=J.device), storage="i8")
        e.init_replicas(G * P, seed=SEED)
        return e

    if a.shape in ("lattice_22", "both"):
        keep("lattice_22", measure("lattice_22", lattice_engine, "sweep_transverse", P * 0.05, 1.0, a))
    if a.shape in ("dense_i8", "both"):
        keep("dense_i8", measure("dense_i8", dense_engine, "sweep_transverse_dense", 30.0, 30.0, a))
    if a.physics:
        doc["physics_lattice_22_%g_%g" % tuple(a.ladder)] = physics(a)
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
