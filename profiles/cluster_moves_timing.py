"""Isoenergetic cluster moves (sga_cluster_move_ladders, csrc/cluster_moves.hip): time of the device call against the host
route it replaces, written to profiles/cluster_moves.json (DESIGN.md "Isoenergetic cluster moves").

The instance: a 3-D +-J lattice of 22^3 = 10 648 spins with periodic boundaries, two copies of a ladder of 512
temperatures from 3 down to 0.2 (1024 replicas), 1200 sweeps with an exchange round every 10 before anything is timed.
Figures, on ONE engine that runs on torch's stream so that torch events bracket its work:
  cluster_all_ms       one cluster_move_ladders() over all 512 slots: median [min, max] of `--reps` (20) calls after
                       `--warmup` (3), event time; the sizes go to a device tensor, so nothing waits on the host
  cluster_cold_ms      ... over the cold half of the ladder (slots 256 ... 511)
  sweep_ms             one sweep of the same engine, same timing
  energy_pass_ms       one recompute_energies(): the part of a cluster call that is not the move
  sizes                mean and largest cluster, share of empty moves, over one call of all slots; bfs_levels: mean and
                       most levels of the search over `--level-pairs` (64) of its pairs, by the host reference
  host_route_ms        what a user did before: spins() of all replicas, per pair the differing sites, one drawn, its
                       component by scipy.sparse.csgraph.connected_components on the induced subgraph (the fastest host
                       search at hand), and two set_spins(); timed on the first `--host-pairs` (32) pairs, the part per
                       pair scaled to 512 (the spins() copy is counted once); the components are compared with the
                       device's through tests/cluster_reference.py
--c3 runs the other measurement: ms per sweep of bench.py's C3 graph (n = 10^4, degree ~32, 4096 replicas), 16 timed
sweeps after 16, kernel time from enable_timing, in a process of its own per run, this library and --baseline-lib (the
parent commit's build, through SGA_LIBRARY_PATH) alternating, three runs each: the one-model line must not move.
`--ab LABEL`: cluster_all_ms and cluster_all_host_sizes_ms (the sizes on the host) alone, of the library in use (SGA_LIBRARY_PATH), appended as one round under
doc["ab_rounds"][LABEL]["lattice_22"] (profiles/ab_rounds.py); nothing else of the file changes.
usage: cluster_moves_timing.py [--reps 20] [--warmup 3] [--c3 --baseline-lib build/libsga_parent.so] [--no-write]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "cluster_moves.json")
LX, SLOTS, COPIES, T_HOT, T_COLD = 22, 512, 2, 3.0, 0.2


def lattice(lx, seed):
    """CSR of the periodic simple-cubic lattice with +-1 couplings, rows sorted by column."""
    import scipy.sparse as sp
    rng = np.random.RandomState(seed)
    x, y, z = np.meshgrid(np.arange(lx), np.arange(lx), np.arange(lx), indexing="ij")
    site = lambda a, b, c: ((a % lx) * lx + (b % lx)) * lx + (c % lx)  # noqa: E731
    i = np.concatenate([site(x, y, z).ravel()] * 3)
    j = np.concatenate([site(x + 1, y, z).ravel(), site(x, y + 1, z).ravel(), site(x, y, z + 1).ravel()])
    v = (rng.randint(0, 2, i.size) * 2 - 1).astype(np.float32)
    A = sp.coo_matrix((v, (i, j)), shape=(lx ** 3, lx ** 3)).tocsr()
    A = (A + A.T).tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float32)


def event_ms(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return [float(np.median(times)), float(min(times)), float(max(times))]


def host_route(e, graph, pairs, seed, rnd, timed_pairs):
    """spins() + per pair a host search + set_spins(): (ms of the copy, ms per pair, the flipped sets)."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    import cluster_reference as cr
    A = sp.csr_matrix((graph[2], graph[1], graph[0]), shape=(e.n, e.n))
    t0 = time.perf_counter()
    S = e.spins()
    t_copy = (time.perf_counter() - t0) * 1e3
    flipped = []
    t0 = time.perf_counter()
    for a, b in pairs[:timed_pairs]:
        sites = np.nonzero(S[a] != S[b])[0]
        if sites.size == 0:
            flipped.append(sites)
            continue
        k = cr.seed_index(seed, rnd, min(a, b), sites.size)
        _, label = connected_components(A[sites][:, sites], directed=False)
        comp = sites[label == label[k]]
        S[a, comp] = -S[a, comp]
        S[b, comp] = -S[b, comp]
        e.set_spins(a, S[a])
        e.set_spins(b, S[b])
        flipped.append(comp)
    return t_copy, (time.perf_counter() - t0) * 1e3 / max(timed_pairs, 1), flipped


def main_cluster(a):
    import torch
    import cluster_reference as cr
    import spin_glass_anneal_rl_amd as sg
    torch.zeros(1, device="cuda")
    torch.cuda.set_stream(torch.cuda.Stream())  # (a stream of its own: handle 0 would mean the engine's own)
    graph = lattice(LX, 1)
    n, R, seed = LX ** 3, COPIES * SLOTS, 42
    temps = np.geomspace(T_HOT, T_COLD, SLOTS)
    res = {"n": n, "replicas": R, "slots": SLOTS, "copies": COPIES, "temperatures": [T_HOT, T_COLD], "warmup": a.warmup, "reps": a.reps}
    with sg.AnnealEngine(0) as e:
        e.use_stream(torch.cuda.current_stream().cuda_stream)
        e.set_csr(*graph, np.zeros(n, np.float32))
        e.init_replicas(R, seed=seed)
        e.set_ladder(np.tile(temps, COPIES), COPIES)
        for _ in range(120):
            e.sweep(10)
            e.exchange(count=False)
        rnd = [100]

        def call(lo, hi, out):
            rnd[0] += 1
            e.cluster_move_ladders(lo, hi, round=rnd[0], sizes=out)
        if a.ab:  # the move of all slots with its sizes left on the device, and with the sizes on the host
            out_all = torch.zeros(SLOTS, dtype=torch.int32, device="cuda")
            figures = {"cluster_all_ms": event_ms(torch, lambda: call(0, SLOTS, out_all), a.warmup, a.reps),
                       "cluster_all_host_sizes_ms": event_ms(torch, lambda: call(0, SLOTS, True), a.warmup, a.reps)}
            return {"figures": figures, "library": os.path.basename(sg._native.library_path())}
        res["describe"] = e.describe()
        res["sweep_ms"] = event_ms(torch, lambda: e.sweep(1), a.warmup, a.reps)
        res["energy_pass_ms"] = event_ms(torch, e.recompute_energies, a.warmup, a.reps)
        # one call of all slots held against the host reference on some of its pairs, and its sizes
        sm, S = e.slot_map(), e.spins()
        pairs = [(int(sm[s]), int(sm[SLOTS + s])) for s in range(SLOTS)]
        sizes = e.cluster_move_ladders(round=100).reshape(-1)
        S1 = e.spins()
        lv = []
        for s in np.linspace(0, SLOTS - 1, a.level_pairs).astype(int):
            p, q = pairs[s]
            cnt = int(np.count_nonzero(S[p] != S[q]))
            if cnt == 0:
                assert sizes[s] == 0
                continue
            k = cr.seed_index(seed, 100, min(p, q), cnt)
            comp = cr.component(*graph, S[p], S[q], k)
            assert comp.size == sizes[s] and np.array_equal(np.nonzero(S1[p] != S[p])[0], comp), s
            lv.append(cr.levels(*graph, S[p], S[q], k))
        res["sizes"] = {"mean": float(sizes.mean()), "max": int(sizes.max()), "empty_share": float(np.mean(sizes == 0)),
                        "mean_cold_half": float(sizes[SLOTS // 2:].mean()), "max_cold_half": int(sizes[SLOTS // 2:].max())}
        res["bfs_levels"] = {"pairs": len(lv), "mean": float(np.mean(lv)), "max": int(max(lv))}
        out_all = torch.zeros(SLOTS, dtype=torch.int32, device="cuda")
        out_cold = torch.zeros(SLOTS // 2, dtype=torch.int32, device="cuda")
        res["cluster_all_ms"] = event_ms(torch, lambda: call(0, SLOTS, out_all), a.warmup, a.reps)
        res["cluster_cold_ms"] = event_ms(torch, lambda: call(SLOTS // 2, SLOTS, out_cold), a.warmup, a.reps)
        # the host route, on a state the device has not yet moved under the round it draws with
        S = e.spins()
        t_copy, t_pair, flipped = host_route(e, graph, pairs, seed, 7, a.host_pairs)
        for (p, q), comp in zip(pairs, flipped):  # the same sets the device flips
            cnt = int(np.count_nonzero(S[p] != S[q]))
            want = cr.component(*graph, S[p], S[q], cr.seed_index(seed, 7, min(p, q), cnt)) if cnt else np.zeros(0, np.int64)
            assert np.array_equal(np.sort(comp), want)
        res["host_route_ms"] = {"spins_copy": t_copy, "per_pair": t_pair, "pairs_timed": a.host_pairs,
                                "all_slots_scaled": t_copy + t_pair * SLOTS, "cold_half_scaled": t_copy + t_pair * SLOTS / 2}
    return res


def c3_worker():
    import ctypes
    import torch
    import bench
    from spin_glass_anneal_rl_amd import _native as N
    if os.environ.get("SGA_LIBRARY_PATH"):  # an older library: bind what it has (the one-model line calls nothing newer)
        have = ctypes.CDLL(N.library_path())
        N.SYMBOLS[:] = [s for s in N.SYMBOLS if hasattr(have, s[0])]
    import spin_glass_anneal_rl_amd as sg
    n, R = 10000, 4096
    with sg.AnnealEngine(0) as e:
        e.set_csr(*bench.make_sparse_instance(n, 16, 3), torch.zeros(n, device="cuda"))
        e.init_replicas(R, seed=42)
        e.set_temperatures(bench.geometric_ladder(R, 10.0, 0.1))
        e.sweep(16)
        e.enable_timing(True)
        e.sweep(16)
        launches, ms = e.kernel_time()
        print(json.dumps({"ms_per_sweep": ms / 16, "kernel": sg.engine.last_kernel(), "version": sg._native.lib().sga_version()}))


def main_c3(a):
    runs = {"this": [], "parent": []}
    for i in range(3):
        for arm in (("parent", "this"), ("this", "parent"))[i % 2]:  # (neither arm always runs first)
            env = dict(os.environ)
            env.pop("SGA_LIBRARY_PATH", None)
            if arm == "parent":
                env["SGA_LIBRARY_PATH"] = os.path.abspath(a.baseline_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--c3-worker"], env=env, capture_output=True, text=True,
                               timeout=240)
            if p.returncode != 0:  # nothing more is started after a failed run
                sys.exit(f"c3 run ({arm}) failed: rc={p.returncode}\n{p.stderr[-2000:]}")
            runs[arm].append(json.loads(p.stdout.strip().splitlines()[-1]))
    out = {}
    for arm, rs in runs.items():
        ms = [r["ms_per_sweep"] for r in rs]
        out[arm] = {"ms_per_sweep": [float(np.median(ms)), float(min(ms)), float(max(ms))], "runs": ms, "kernel": rs[0]["kernel"],
                    "version": rs[0]["version"]}
    lo, hi = out["parent"]["ms_per_sweep"][1:]
    out["this_median_inside_parent_spread"] = bool(lo <= out["this"]["ms_per_sweep"][0] <= hi)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--level-pairs", type=int, default=64)
    ap.add_argument("--host-pairs", type=int, default=32)
    ap.add_argument("--c3", action="store_true")
    ap.add_argument("--c3-worker", action="store_true")
    ap.add_argument("--baseline-lib", default=os.path.join(ROOT, "build", "libsga_parent.so"))
    ap.add_argument("--ab", default="", metavar="LABEL")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.c3_worker:
        c3_worker()
        sys.exit(0)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    if a.c3:
        doc["c3_one_model_line"] = main_c3(a)
    elif a.ab:
        import ab_rounds
        got = main_cluster(a)
        ab_rounds.append(doc, a.ab, "lattice_22", got["figures"], got["library"])
    else:
        doc["lattice_22"] = main_cluster(a)
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
