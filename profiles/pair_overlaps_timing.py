"""Spin and link overlaps between ladder copies (sga_accumulate_ladder_overlaps, csrc/pair_overlaps.hip): time of the device
call against a sweep, against overlaps() and against the host route it replaces, written to profiles/pair_overlaps.json
(DESIGN.md "Spin and link overlaps between pairs").

Two shapes, each one engine on torch's stream so that torch events bracket its work, two copies of a ladder 3 -> 0.2:
  lattice_22   a 3-D +-J lattice of 22^3 = 10 648 spins with periodic boundaries, 2 x 512 replicas, 1200 sweeps with an
               exchange round every 10 before anything is timed (the shape of profiles/cluster_moves.json)
  c3           bench.py's C3 graph (n = 10^4, degree ~32), 2 x 2048 replicas, 200 sweeps with an exchange every 10
Figures per shape, median [min, max] ms of `--reps` (20) calls after `--warmup` (3), event time:
  ladder_links_ms      one accumulate_ladder_overlaps() over all slots into hist_q and hist_l (bins of a power-of-two
                       width, at most 4096 a cell: the time does not depend on the bins)
  ladder_spins_ms      ... into hist_q alone (no bitmap, no walk)
  sweep_ms             one sweep of the same engine
  overlaps_device_ms   overlaps(out=<device tensor>): all R^2 entries for the R / 2 that are wanted
  link_count_ms        one link_count() (host clocked: it returns a number)
  host_route_ms        what a user did before: spins() and slot_map() (host clocked), then per pair a numpy count over
                       the stored entries, timed on the first `--host-pairs` (32) pairs and scaled to all slots; the counts
                       are compared with one device call's histograms through tests/overlap_reference.py
`--ab LABEL`: ladder_links_ms, ladder_spins_ms, link_count_ms and pairs_host_ms (the pair form of --host-pairs pairs, results on the host) alone, of the library in use (SGA_LIBRARY_PATH), appended as one round under
doc["ab_rounds"][LABEL][shape] (profiles/ab_rounds.py); nothing else of the file changes.
usage: pair_overlaps_timing.py [--reps 20] [--warmup 3] [--shape lattice_22|c3|both] [--out FILE] [--no-write]"""
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
OUT = os.path.join(ROOT, "profiles", "pair_overlaps.json")
COPIES, T_HOT, T_COLD, MAX_BINS = 2, 3.0, 0.2, 4096


def host_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(times)), float(min(times)), float(max(times))]


def measure(name, graph, slots, presweeps, a):
    import torch
    import overlap_reference as ovr
    import spin_glass_anneal_rl_amd as sg
    from cluster_moves_timing import event_ms
    from spin_glass_anneal_rl_amd.parallel_tempering import bin_shift
    n, R, seed = len(graph[0]) - 1, COPIES * slots, 42
    temps = np.geomspace(T_HOT, T_COLD, slots)
    res = {"n": n, "replicas": R, "slots": slots, "copies": COPIES, "temperatures": [T_HOT, T_COLD], "warmup": a.warmup,
           "reps": a.reps, "presweeps": presweeps}
    with sg.AnnealEngine(0) as e:
        e.use_stream(torch.cuda.current_stream().cuda_stream)
        e.set_csr(*graph, np.zeros(n, np.float32))
        e.init_replicas(R, seed=seed)
        e.set_ladder(np.tile(temps, COPIES), COPIES)
        for _ in range(presweeps // 10):
            e.sweep(10)
            e.exchange(count=False)
        res["describe"] = e.describe()
        links = e.link_count()
        qs, ls = bin_shift(n, MAX_BINS), bin_shift(links, MAX_BINS)
        res.update(links=links, entries=int(len(graph[1])), q_shift=qs, l_shift=ls)
        hq = torch.zeros((1, slots, (n >> qs) + 1), dtype=torch.int64, device="cuda")
        hl = torch.zeros((1, slots, (links >> ls) + 1), dtype=torch.int64, device="cuda")
        # one call held against the host reference on the timed pairs, which is the host route's count
        e.accumulate_ladder_overlaps(hq, hl, q_shift=qs, l_shift=ls)
        torch.cuda.synchronize()
        got_q, got_l = hq.cpu().numpy()[0], hl.cpu().numpy()[0]
        t0 = time.perf_counter()
        S = e.spins()
        t_spins = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        sm = e.slot_map()
        t_map = (time.perf_counter() - t0) * 1e3
        row, col = ovr.links(*graph)
        t0 = time.perf_counter()
        counted = []
        for s in range(a.host_pairs):
            x = S[sm[s]] != S[sm[slots + s]]
            counted.append((int(np.count_nonzero(x)), int(np.count_nonzero(x[row] != x[col]))))
        t_pair = (time.perf_counter() - t0) * 1e3 / max(a.host_pairs, 1)
        for s, (d, b) in enumerate(counted):
            assert got_q[s, d >> qs] == 1 and got_q[s].sum() == 1 and got_l[s, b >> ls] == 1 and got_l[s].sum() == 1, s
        if a.ab:  # the device calls, and the two whose results land on the host
            pairs = np.stack([sm[:slots], sm[slots:]], axis=1)[:a.host_pairs]
            figures = {"ladder_links_ms": event_ms(torch, lambda: e.accumulate_ladder_overlaps(hq, hl, q_shift=qs, l_shift=ls), a.warmup, a.reps),
                       "ladder_spins_ms": event_ms(torch, lambda: e.accumulate_ladder_overlaps(hq, q_shift=qs), a.warmup, a.reps),
                       "link_count_ms": host_ms(e.link_count, a.warmup, a.reps),
                       "pairs_host_ms": host_ms(lambda: e.pair_overlaps(pairs), a.warmup, a.reps)}
            return {"figures": figures, "library": os.path.basename(sg._native.library_path())}
        res["host_route_ms"] = {"spins_copy": t_spins, "slot_map": t_map, "per_pair": t_pair, "pairs_timed": a.host_pairs,
                                "all_slots_scaled": t_spins + t_map + t_pair * slots}
        res["spins_ms"] = host_ms(e.spins, 1, 5)
        res["sweep_ms"] = event_ms(torch, lambda: e.sweep(1), a.warmup, a.reps)
        res["ladder_links_ms"] = event_ms(torch, lambda: e.accumulate_ladder_overlaps(hq, hl, q_shift=qs, l_shift=ls), a.warmup, a.reps)
        res["ladder_spins_ms"] = event_ms(torch, lambda: e.accumulate_ladder_overlaps(hq, q_shift=qs), a.warmup, a.reps)
        Q = torch.zeros((R, R), dtype=torch.int32, device="cuda")
        res["overlaps_device_ms"] = event_ms(torch, lambda: e.overlaps(out=Q), a.warmup, a.reps)
        res["link_count_ms"] = host_ms(e.link_count, a.warmup, a.reps)
        torch.cuda.synchronize()
        assert int(hq.sum()) == slots * (1 + 2 * (a.warmup + a.reps)) and int(hl.sum()) == slots * (1 + a.warmup + a.reps)
    res["ladder_links_over_sweep"] = res["ladder_links_ms"][0] / res["sweep_ms"][0]
    res["ladder_links_over_spins"] = res["ladder_links_ms"][0] / res["spins_ms"][0]
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-pairs", type=int, default=32)
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
    def keep(shape, got):
        if a.ab:
            import ab_rounds
            ab_rounds.append(doc, a.ab, shape, got["figures"], got["library"])
        else:
            doc[shape] = got

    if a.shape in ("lattice_22", "both"):
        from cluster_moves_timing import lattice
        keep("lattice_22", measure("lattice_22", lattice(22, 1), 512, 1200, a))
    if a.shape in ("c3", "both"):
        import bench
        keep("c3", measure("c3", bench.make_sparse_instance(10000, 16, 3), 2048, 200, a))
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
