"""Class-resolved overlaps between ladder copies (sga_accumulate_ladder_class_overlaps, csrc/class_overlaps.hip): time of the
device call against a sweep, against the plain ladder overlaps and against the host route it replaces, written to
profiles/class_overlaps.json (DESIGN.md "Class-resolved overlaps").

Two shapes, each one engine on torch's stream so that torch events bracket its work, two copies of a ladder 3 -> 0.2 (the
shapes of profiles/pair_overlaps.json):
  lattice_22   a 3-D +-J lattice of 22^3 = 10 648 spins with periodic boundaries, 2 x 512 replicas, 1200 sweeps with an
               exchange round every 10 before anything is timed; the three plane maps of lattice_planes((22, 22, 22)), C = 22
  c3           bench.py's C3 graph (n = 10^4, degree ~32), 2 x 2048 replicas, 200 sweeps with an exchange every 10; one map
               of 100 random classes
Figures per shape, median [min, max] ms of `--reps` (20) calls after `--warmup` (3), event time:
  ladder_sum12_ms      one accumulate_ladder_class_overlaps() over all slots into sum1 and sum2
  ladder_sum1_ms       ... into sum1 alone
  one_class_sum1_ms    ... with one map that puts every site into one class (C = 1): every lane on one counter
  pair_form_device_ms  class_overlaps(pairs of the slot map, device map, out=<device tensor>): the pair list staged, no sums
  sweep_ms             one sweep of the same engine
  ladder_overlaps_ms   accumulate_ladder_overlaps() without links (the distance alone, csrc/pair_overlaps.hip)
  spins_ms             spins() alone (host clocked)
  host_route_ms        what a user did before: spins() and slot_map() (host clocked), then per pair and map an np.bincount
                       over the differing sites, timed on the first `--host-pairs` (32) pairs and scaled to all slots; the
                       counts are compared with one device call's sums
`--variant NAME`: only the three ladder figures, stored under <shape>.variants.NAME -- for a library in SGA_LIBRARY_PATH whose
class_overlaps.hip was compiled with -DSGA_CLASS_OVERLAP_SHORTCUT=0 | 1 (the ballot shortcut) and
-DSGA_CLASS_OVERLAP_MAX_COPIES=1 | 4 (the copies of the counters) and linked with the other objects as they are; the
committed file holds all four as shortcut<S>_copies<K>.
`--ab LABEL`: ladder_sum12_ms, ladder_sum1_ms and pair_form_host_ms (the pair form of --host-pairs pairs, map and result on the host) alone, of the library in use (SGA_LIBRARY_PATH), appended as one round under
doc["ab_rounds"][LABEL][shape] (profiles/ab_rounds.py); nothing else of the file changes.
usage: class_overlaps_timing.py [--reps 20] [--warmup 3] [--shape lattice_22|c3|both] [--variant NAME] [--out FILE] [--no-write]"""
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
OUT = os.path.join(ROOT, "profiles", "class_overlaps.json")
COPIES, T_HOT, T_COLD = 2, 3.0, 0.2


def host_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(times)), float(min(times)), float(max(times))]


def measure(name, graph, classes, n_classes, slots, presweeps, a):
    import torch
    import spin_glass_anneal_rl_amd as sg
    from cluster_moves_timing import event_ms
    n, R, seed = len(graph[0]) - 1, COPIES * slots, 42
    M = classes.shape[0]
    temps = np.geomspace(T_HOT, T_COLD, slots)
    res = {"n": n, "replicas": R, "slots": slots, "copies": COPIES, "temperatures": [T_HOT, T_COLD], "warmup": a.warmup,
           "reps": a.reps, "presweeps": presweeps, "n_maps": M, "n_classes": n_classes, "library": os.path.basename(sg._native.library_path())}
    with sg.AnnealEngine(0) as e:
        e.use_stream(torch.cuda.current_stream().cuda_stream)
        e.set_csr(*graph, np.zeros(n, np.float32))
        e.init_replicas(R, seed=seed)
        e.set_ladder(np.tile(temps, COPIES), COPIES)
        for _ in range(presweeps // 10):
            e.sweep(10)
            e.exchange(count=False)
        dmap = torch.from_numpy(classes).cuda()
        s1 = torch.zeros((1, slots, M, n_classes), dtype=torch.int64, device="cuda")
        s2 = torch.zeros((1, slots, M, n_classes, n_classes), dtype=torch.int64, device="cuda")
        # one call held against the host route's counts on the timed pairs
        e.accumulate_ladder_class_overlaps(dmap, n_classes, s1, s2)
        torch.cuda.synchronize()
        got1, got2 = s1.cpu().numpy()[0], s2.cpu().numpy()[0]
        t0 = time.perf_counter()
        S = e.spins()
        t_spins = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        sm = e.slot_map()
        t_map = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        counted = []
        for s in range(a.host_pairs):
            x = S[sm[s]] != S[sm[slots + s]]
            counted.append(np.stack([np.bincount(classes[m][x], minlength=n_classes) for m in range(M)]))
        t_pair = (time.perf_counter() - t0) * 1e3 / max(a.host_pairs, 1)
        for s, D in enumerate(counted):
            assert np.array_equal(got1[s], D) and np.array_equal(got2[s], D[:, :, None] * D[:, None, :]), s
        res["differing_share_hot_cold"] = [float(got1[0, 0].sum()) / n, float(got1[-1, 0].sum()) / n]
        ladder12 = event_ms(torch, lambda: e.accumulate_ladder_class_overlaps(dmap, n_classes, s1, s2), a.warmup, a.reps)
        ladder1 = event_ms(torch, lambda: e.accumulate_ladder_class_overlaps(dmap, n_classes, s1), a.warmup, a.reps)
        # every site in one class: all lanes of all waves on one counter, the greatest contention a map can ask for
        zmap = torch.zeros((1, n), dtype=torch.int32, device="cuda")
        z1 = torch.zeros((1, slots, 1, 1), dtype=torch.int64, device="cuda")
        one_class = event_ms(torch, lambda: e.accumulate_ladder_class_overlaps(zmap, 1, z1), a.warmup, a.reps)
        if a.ab:  # the two ladder calls, and the pair form with its result on the host
            pairs = np.stack([sm[:slots], sm[slots:]], axis=1)[:a.host_pairs]
            figures = {"ladder_sum12_ms": ladder12, "ladder_sum1_ms": ladder1,
                       "pair_form_host_ms": host_ms(lambda: e.class_overlaps(pairs, classes, n_classes), a.warmup, a.reps)}
            return {"figures": figures, "library": res["library"]}
        if a.variant:
            return {"ladder_sum12_ms": ladder12, "ladder_sum1_ms": ladder1, "one_class_sum1_ms": one_class, "library": res["library"]}
        res["ladder_sum12_ms"], res["ladder_sum1_ms"], res["one_class_sum1_ms"] = ladder12, ladder1, one_class
        res["host_route_ms"] = {"spins_copy": t_spins, "slot_map": t_map, "per_pair": t_pair, "pairs_timed": a.host_pairs,
                                "all_slots_scaled": t_spins + t_map + t_pair * slots}
        res["describe"] = e.describe()
        pairs = np.stack([sm[:slots], sm[slots:]], axis=1)
        D = torch.zeros((slots, M, n_classes), dtype=torch.int32, device="cuda")
        res["pair_form_device_ms"] = event_ms(torch, lambda: e.class_overlaps(pairs, dmap, n_classes, out=D), a.warmup, a.reps)
        torch.cuda.synchronize()
        assert np.array_equal(D.cpu().numpy(), got1)
        res["spins_ms"] = host_ms(e.spins, 1, 5)
        hq = torch.zeros((1, slots, n + 1), dtype=torch.int64, device="cuda")
        res["ladder_overlaps_ms"] = event_ms(torch, lambda: e.accumulate_ladder_overlaps(hq), a.warmup, a.reps)
        res["sweep_ms"] = event_ms(torch, lambda: e.sweep(1), a.warmup, a.reps)
        torch.cuda.synchronize()
    res["bytes_per_call"] = slots * (2 * n + 4 * M * n)
    res["ladder_sum12_over_sweep"] = res["ladder_sum12_ms"][0] / res["sweep_ms"][0]
    res["ladder_sum12_over_spins"] = res["ladder_sum12_ms"][0] / res["spins_ms"][0]
    res["ladder_sum12_over_ladder_overlaps"] = res["ladder_sum12_ms"][0] / res["ladder_overlaps_ms"][0]
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-pairs", type=int, default=32)
    ap.add_argument("--shape", default="both", choices=["lattice_22", "c3", "both"])
    ap.add_argument("--variant", default=None)
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

    def keep(shape, res):
        if a.ab:
            import ab_rounds
            ab_rounds.append(doc, a.ab, shape, res["figures"], res["library"])
        elif a.variant:
            doc.setdefault(shape, {}).setdefault("variants", {})[a.variant] = res
        else:
            res["variants"] = doc.get(shape, {}).get("variants", {})
            doc[shape] = res

    if a.shape in ("lattice_22", "both"):
        from cluster_moves_timing import lattice
        from spin_glass_anneal_rl_amd.encoders import lattice_planes
        keep("lattice_22", measure("lattice_22", lattice(22, 1), lattice_planes((22, 22, 22)), 22, 512, 1200, a))
    if a.shape in ("c3", "both"):
        import bench
        classes = np.random.RandomState(7).randint(0, 100, (1, 10000)).astype(np.int32)
        keep("c3", measure("c3", bench.make_sparse_instance(10000, 16, 3), classes, 100, 2048, 200, a))
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
