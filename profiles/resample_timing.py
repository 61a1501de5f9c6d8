"""Population annealing's resampling step (sga_resample, csrc/resample.hip): time of the device call against the host
route it replaces, written to profiles/resample.json (DESIGN.md "Population annealing: resampling on the device").

Instances: "lattice" -- a 3-D +-J lattice of 22^3 = 10 648 spins as CSR, 4096 replicas at T = 1.5; "dense" -- the dense
+-1 model of 10^4 spins, 1024 replicas at T = 100.  One population.  Steps: dbeta found by bisection on the energies
(tests/resample_reference.py) so that about 0.8 and about 0.3 of the slots survive -- first on the equilibrated ones, then
four times more on those of the regime the timed calls run in, a call every two sweeps.  One process per cell
(instance x step); event time, median [min, max] of `--reps` (20) after `--warmup` (3); two sweeps between two timed calls
spread the energies again, so every call does about the same work (the achieved survivor share is recorded).
  resample_device_ms  sga_resample with three device outputs: nothing waits on the host
  resample_host_ms    ... with three host outputs (event time; wall_ms: host clock around the call)
  plan_ms             the call at dbeta = 0: the plan kernel runs in full, the copy kernel finds nothing to copy;
                      copy_ms = resample_device_ms - plan_ms
  copy_gb_per_s       (rows read + rows written, spins and, where the best followed, best spins) / copy_ms, beside
                      probe_read_gb_per_s, the streaming-read probe
  sweep_ms            one sweep of the same engine
  reseed              field cache ON: the first sweep after a call (the cached fields are seeded again) and a later one
  host_route_ms       what a user did before: energies(), a numpy plan, spins(), one set_spins() per overwritten slot --
                      the set_spins() part timed on the first `--host-slots` (64) of them and scaled
`--ab LABEL`: resample_device_ms and resample_host_ms per cell alone, of the library in use (SGA_LIBRARY_PATH), appended as one round under
doc["ab_rounds"][LABEL][cell] (profiles/ab_rounds.py); nothing else of the file changes.
usage: resample_timing.py [--reps 20] [--warmup 3] [--no-write]      (the driver; --cell INSTANCE:SHARE runs one cell)"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "resample.json")
CELLS = [("lattice", 0.8), ("lattice", 0.3), ("dense", 0.8), ("dense", 0.3)]
SEED = 42


def setup(sg, torch, instance, cache):
    from cluster_moves_timing import lattice
    e = sg.AnnealEngine(0)
    e.use_stream(torch.cuda.current_stream().cuda_stream)
    e.set_field_cache("on" if cache else "off")
    if instance == "lattice":
        graph = lattice(22, 1)
        n, R, T, warm = 22 ** 3, 4096, 1.5, 60
        e.set_csr(*graph, np.zeros(n, np.float32))
    else:
        n, R, T, warm = 10000, 1024, 100.0, 20
        g = torch.Generator(device="cuda").manual_seed(1)
        J = torch.triu((torch.randint(0, 2, (n, n), device="cuda", generator=g) * 2 - 1).float(), 1)
        e.set_dense(J + J.T, torch.zeros(n, device="cuda"))
        del J
    e.init_replicas(R, seed=SEED)
    e.set_temperatures(T)
    e.sweep(warm)
    return e, n, R


def event_ms(torch, fn, warmup, reps, between=None):
    times = []
    for i in range(warmup + reps):
        if between is not None:
            between()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        if i >= warmup:
            times.append(t0.elapsed_time(t1))
    return [float(np.median(times)), float(min(times)), float(max(times))]


def survivors(E, dbeta, rnd):
    import resample_reference as rr
    par = rr.plan(E, dbeta, SEED, rnd, 0)[0]
    return float(np.mean(par == np.arange(par.size)))


def find_dbeta(E, share):
    """dbeta > 0 with about `share` of the slots surviving (bisection; the share falls as dbeta grows)."""
    lo, hi = 0.0, 8.0 / max(float(np.std(E)), 1e-9)
    for _ in range(18):
        mid = 0.5 * (lo + hi)
        if survivors(E, mid, 0) > share:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def numpy_plan(E, dbeta, u):
    """The host's plan in floating point: systematic resampling, survivors stay (what a user's numpy step does)."""
    N = E.size
    w = np.exp(-dbeta * (E - E.min()))
    c = np.cumsum(w)
    parent_of_child = np.searchsorted(c, (np.arange(N) + u) * (c[-1] / N), side="right").clip(0, N - 1)
    counts = np.bincount(parent_of_child, minlength=N)
    parents = np.arange(N)
    parents[counts == 0] = np.repeat(np.arange(N), np.maximum(counts - 1, 0))
    return parents


def cell(instance, share, a):
    import torch
    import spin_glass_anneal_rl_amd as sg
    from spin_glass_anneal_rl_amd import _native as N
    torch.zeros(1, device="cuda")
    torch.cuda.set_stream(torch.cuda.Stream())  # (a stream of its own: handle 0 would mean the engine's own)
    res = {"instance": instance, "target_survivor_share": share, "warmup": a.warmup, "reps": a.reps,
           "library_version": int(N.lib().sga_version())}
    e, n, R = setup(sg, torch, instance, cache=False)
    with e:
        res.update(n=n, replicas=R, describe=e.describe())
        E = e.energies()
        dbeta = find_dbeta(E, share)
        res["energy_std"] = float(np.std(E))
        # the timed calls follow one another two sweeps apart: find dbeta again on the energies of that regime
        for _ in range(4):
            e.resample(dbeta, parents=False)
            e.sweep(2)
            dbeta = find_dbeta(e.energies(), share)
        res["dbeta"] = dbeta
        par_d = torch.zeros(R, dtype=torch.int32, device="cuda")
        shift_d = torch.zeros(1, dtype=torch.float64, device="cuda")
        sum_d = torch.zeros(1, dtype=torch.int64, device="cuda")
        par_h, shift_h, sum_h = np.zeros(R, np.int32), np.zeros(1), np.zeros(1, np.uint64)
        db = np.asarray([dbeta]), np.asarray([0.0])
        rnd, shares, wall = [0], [], []

        def call(dbv, device):
            rnd[0] += 1
            p = (C.c_void_p(par_d.data_ptr()), C.c_void_p(shift_d.data_ptr()), C.c_void_p(sum_d.data_ptr())) if device else \
                (par_h.ctypes.data_as(C.c_void_p), shift_h.ctypes.data_as(C.c_void_p), sum_h.ctypes.data_as(C.c_void_p))
            t0 = time.perf_counter()
            N.check(e._lib.sga_resample(e._h, 1, dbv.ctypes.data_as(C.c_void_p), rnd[0], *p), "sga_resample")
            wall.append((time.perf_counter() - t0) * 1e3)

        def spread():  # (also notes what the last timed call left)
            if rnd[0]:
                shares.append(float((par_d.cpu().numpy() == np.arange(R)).mean()))
            e.sweep(2)
        if a.ab:  # the call with its results left on the device, and with them on the host
            figures = {"resample_device_ms": event_ms(torch, lambda: call(db[0], True), a.warmup, a.reps, between=lambda: e.sweep(2)),
                       "resample_host_ms": event_ms(torch, lambda: call(db[0], False), a.warmup, a.reps, between=lambda: e.sweep(2))}
            return {"figures": figures, "library": os.path.basename(N.library_path())}
        res["sweep_ms"] = event_ms(torch, lambda: e.sweep(1), a.warmup, a.reps)
        res["resample_device_ms"] = event_ms(torch, lambda: call(db[0], True), a.warmup, a.reps, between=spread)
        spread()
        res["survivor_share"] = [float(np.mean(shares[1:])), float(min(shares[1:])), float(max(shares[1:]))]
        res["plan_ms"] = event_ms(torch, lambda: call(db[1], True), a.warmup, a.reps, between=lambda: e.sweep(2))
        wall.clear()
        res["resample_host_ms"] = event_ms(torch, lambda: call(db[0], False), a.warmup, a.reps, between=lambda: e.sweep(2))
        res["resample_host_wall_ms"] = [float(np.median(wall[a.warmup:])), float(min(wall[a.warmup:])), float(max(wall[a.warmup:]))]
        res["copy_ms"] = res["resample_device_ms"][0] - res["plan_ms"][0]
        # the bytes one call moves: an overwritten slot's row read and written, and written again where the best followed
        e.sweep(2)
        before_best = np.asarray([e.best(r, with_spins=False)[0] for r in range(R)])
        E = e.energies()
        call(db[0], False)
        moved = par_h != np.arange(R)
        best_rows = int(np.count_nonzero(moved & (E[par_h] < before_best)))
        row = (n + 15) // 16 * 16
        res["copied_rows"], res["best_rows"] = int(moved.sum()), best_rows
        res["copy_bytes"] = (2 * int(moved.sum()) + best_rows) * row
        res["copy_gb_per_s"] = res["copy_bytes"] / max(res["copy_ms"], 1e-6) / 1e6
        res["probe_read_gb_per_s"] = sg.engine.probe_read_bandwidth(0, 1 << 30, 4)
        # the host route on the same engine
        e.sweep(2)
        t0 = time.perf_counter()
        E = e.energies()
        t_e = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        parents = numpy_plan(E, dbeta, 0.5)
        t_plan = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        S = e.spins()
        t_s = (time.perf_counter() - t0) * 1e3
        dst = np.nonzero(parents != np.arange(R))[0]
        t0 = time.perf_counter()
        for d in dst[:a.host_slots]:
            e.set_spins(int(d), S[parents[d]])
        t_set = (time.perf_counter() - t0) * 1e3 / max(min(a.host_slots, dst.size), 1)
        res["host_route_ms"] = {"energies": t_e, "numpy_plan": t_plan, "spins_copy": t_s, "set_spins_per_slot": t_set,
                                "slots_timed": int(min(a.host_slots, dst.size)), "slots_overwritten": int(dst.size),
                                "total_scaled": t_e + t_plan + t_s + t_set * dst.size}
    # the cost of seeding the cached fields again: field cache ON, the first sweep after a call against a later one
    e, n, R = setup(sg, torch, instance, cache=True)
    with e:
        db1, rnd2 = np.asarray([dbeta]), [1000]

        def resample_then(k):
            rnd2[0] += 1
            N.check(e._lib.sga_resample(e._h, 1, db1.ctypes.data_as(C.c_void_p), rnd2[0], None, None, None), "sga_resample")
            if k:
                e.sweep(k)
        res["reseed"] = {"describe": e.describe(),
                         "first_sweep_after_ms": event_ms(torch, lambda: e.sweep(1), a.warmup, a.reps, between=lambda: resample_then(0)),
                         "later_sweep_ms": event_ms(torch, lambda: e.sweep(1), a.warmup, a.reps, between=lambda: resample_then(2))}
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-slots", type=int, default=64)
    ap.add_argument("--cell", default=None)
    ap.add_argument("--ab", default="", metavar="LABEL")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.cell:
        inst, share = a.cell.split(":")
        print(json.dumps(cell(inst, float(share), a)))
        sys.exit(0)
    doc = {}
    if a.ab and os.path.exists(a.out):  # the rounds alone, into the file as it stands
        with open(a.out) as f:
            doc = json.load(f)
    for inst, share in CELLS:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--cell", f"{inst}:{share}", "--reps", str(a.reps), "--warmup",
                            str(a.warmup), "--host-slots", str(a.host_slots)] + (["--ab", a.ab] if a.ab else []),
                           capture_output=True, text=True, timeout=420)
        if p.returncode != 0:  # nothing more is started after a failed cell
            sys.exit(f"cell {inst}:{share} failed: rc={p.returncode}\n{p.stderr[-3000:]}")
        got = json.loads(p.stdout.strip().splitlines()[-1])
        if a.ab:
            import ab_rounds
            ab_rounds.append(doc, a.ab, f"{inst}_survive_{share}", got["figures"], got["library"])
            print(f"{inst}:{share} [{a.ab}]: " + json.dumps(got["figures"]), flush=True)
            continue
        doc[f"{inst}_survive_{share}"] = got
        print(json.dumps(doc[f"{inst}_survive_{share}"], indent=1), flush=True)
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
