"""Replica observables (sga_get_overlaps / sga_get_magnetizations, csrc/observables.hip): time of the device calls
against what a user did before them -- all R n spin bytes to the host, reduced there -- written to
profiles/observables.json (DESIGN.md "Replica observables").

Shapes (bench.py's instances):
  c2a         dense +-1, n = 10^4, R = 1024
  c3          CSR degree ~32, n = 10^4, R = 4096
  c5_1000     the implicit TSP form at 1000 cities (n = 10^6), R = 256 as the bench line runs it
Figures per shape, each the median of `--reps` (default 20) calls after `--warmup` (default 3), host clock around a call
that ends in a synchronisation, on ONE engine in ONE process:
  overlaps_ms               e.overlaps(): the result lands in host memory
  overlaps_device_out_ms    e.overlaps(out=<int32 CUDA tensor>), waited for
  magnetizations_ms         e.magnetizations()
  a_spins_ms                e.spins() alone: the floor of every host route
  b_spins_numpy_int32_ms    e.spins() followed by an int32 numpy product.  The product is minutes long at these shapes,
                            so it is timed on the first `rows` replicas against all R (rows: as many as keep it under
                            ~4 10^9 multiply-adds) and scaled by R / rows; "b_rows_timed" says how many, "b_reps" how often
  c_spins_torch_f32_ms      e.spins(), the array moved back onto the device with torch, a float32 matmul, waited for
The three routes must agree: the device result is compared with (c) in full and with (b) on its rows.
Each shape runs in a process of its own under a time limit; after a failed shape nothing more is started.
`--ab LABEL`: overlaps_ms, overlaps_device_out_ms and magnetizations_ms alone, of the library in use (SGA_LIBRARY_PATH), appended as one round under
doc["ab_rounds"][LABEL][shape] (profiles/ab_rounds.py); nothing else of the file changes.
usage: observables_timing.py [--reps 20] [--warmup 3] [--shapes c2a,c3,c5_1000] [--ab LABEL] [--no-write]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
OUT = os.path.join(ROOT, "profiles", "observables.json")
SHAPES = {"c2a": (10000, 1024), "c3": (10000, 4096), "c5_1000": (1000 * 1000, 256)}
B_MACS = 4e9  # multiply-adds of the int32 numpy product that is actually timed


def load(torch, e, shape):
    import bench
    from spin_glass_anneal_rl_amd import encoders as enc
    n, R = SHAPES[shape]
    if shape == "c2a":
        e.set_dense(bench.make_sk_instance(n, 2, "cuda"), torch.zeros(n, device="cuda"))
        temps = bench.geometric_ladder(R, 10.0, 0.1)
    elif shape == "c3":
        e.set_csr(*bench.make_sparse_instance(n, 16, 3), torch.zeros(n, device="cuda"))
        temps = bench.geometric_ladder(R, 10.0, 0.1)
    else:
        xy = np.random.RandomState(5).rand(1000, 2) * 100.0
        dmat = np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1])
        d32, w_city, w_pos, h, _ = enc.tsp_structure(dmat, 200.0, 200.0)
        e.set_tsp(torch.from_numpy(d32).cuda(), w_city, w_pos, torch.from_numpy(h).cuda())
        temps = np.tile(bench.geometric_ladder(64, 200.0, 2.0), R // 64)
    e.init_replicas(R, seed=42)
    e.set_temperatures(temps)
    return n, R


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


def worker(shape, warmup, reps, ab=False):
    import torch
    import spin_glass_anneal_rl_amd as sg
    torch.zeros(1, device="cuda")
    with sg.AnnealEngine(0) as e:
        n, R = load(torch, e, shape)
        e.sweep(2)  # (a state a run would be in: not the initial draw)
        res = {"n": n, "R": R, "describe": e.describe(), "warmup": warmup, "reps": reps,
               "plan": dict(zip(("tiles_m", "tiles_n", "ksplit", "kchunk"), plan_of(n, R)))}
        out_dev = torch.empty((R, R), dtype=torch.int32, device="cuda")

        def device_out():
            e.overlaps(out=out_dev)
            torch.cuda.synchronize()

        def via_torch():
            X = torch.from_numpy(e.spins()).cuda().float()
            Q = X @ X.T
            torch.cuda.synchronize()
            return Q

        if ab:
            calls = (("overlaps_ms", e.overlaps), ("overlaps_device_out_ms", device_out), ("magnetizations_ms", e.magnetizations))
            return {"figures": {key: list(median_ms(fn, warmup, reps)) for key, fn in calls},
                    "library": os.path.basename(sg._native.library_path())}
        for key, fn in (("overlaps_ms", e.overlaps), ("overlaps_device_out_ms", device_out),
                        ("magnetizations_ms", e.magnetizations), ("a_spins_ms", e.spins), ("c_spins_torch_f32_ms", via_torch)):
            res[key], res[key + "_min"], res[key + "_max"] = median_ms(fn, warmup, reps)
        # (b): the product on `rows` replicas against all, scaled
        rows = int(max(1, min(R, B_MACS // (float(R) * n))))
        S = e.spins()
        t0 = time.perf_counter()
        Qb = S[:rows].astype(np.int32) @ S.astype(np.int32).T
        one = (time.perf_counter() - t0) * 1e3
        b_reps = reps if one * reps < 20e3 else 1
        prod = one if b_reps == 1 else median_ms(lambda: S[:rows].astype(np.int32) @ S.astype(np.int32).T, 0, b_reps)[0]
        res.update(b_spins_numpy_int32_ms=res["a_spins_ms"] + prod * R / rows, b_rows_timed=rows, b_reps=b_reps,
                   b_product_ms_on_rows=prod)
        # the routes agree (fp32 sums of +-1 are exact below 2^24 terms)
        Q = e.overlaps()
        assert np.array_equal(Q, via_torch().cpu().numpy().astype(np.int64)), "device product and fp32 matmul differ"
        assert np.array_equal(Q[:rows], Qb), "device product and numpy product differ"
        assert np.array_equal(out_dev.cpu().numpy(), Q)
        assert np.array_equal(e.magnetizations(), S.astype(np.int64).sum(1))
        res["routes_agree"] = True
    return res


def plan_of(n, R, cus=256):
    """observables_plan (csrc/sga_replicas.h), restated: tests/test_observables_host.py pins it."""
    tiles = -(-R // 128)
    s = min(-(-2 * cus // (tiles * tiles)), -(-n // 512))
    per = -(-n // s)
    kchunk = -(-per // 128) * 128
    return tiles, tiles, -(-n // kchunk), kchunk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--limit", type=int, default=400, help="seconds a shape's process may take")
    ap.add_argument("--ab", default="", metavar="LABEL")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--worker")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.reps < 20 and not a.no_write:
        sys.exit("a written result is a median of at least 20 (use --no-write for a shorter trial)")
    if a.worker:
        res = worker(a.worker, a.warmup, a.reps, bool(a.ab))
        with open(a.out, "w") as f:
            json.dump(res, f)
        return
    import torch
    import spin_glass_anneal_rl_amd as sg
    out = {"device": torch.cuda.get_device_name(0), "library_version": int(sg._native.lib().sga_version()),
           "note": "ms per call: median of `reps` host-clocked calls after `warmup`, each ending in a synchronisation; "
                   "b = a + the int32 numpy product timed on b_rows_timed replicas against all, scaled by R / b_rows_timed"}
    rounds = []
    fd, tmp = tempfile.mkstemp(suffix=".json")
    os.close(fd)
    for shape in a.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", shape, "--out", tmp, "--reps", str(a.reps), "--warmup",
               str(a.warmup)] + (["--no-write"] if a.no_write else []) + (["--ab", a.ab] if a.ab else [])
        proc = subprocess.run(cmd, timeout=a.limit)
        if proc.returncode != 0:  # (nothing more is started on the device after a failed shape)
            sys.exit(f"shape {shape} failed with status {proc.returncode}")
        with open(tmp) as f:
            out[shape] = json.load(f)
        if a.ab:
            rounds.append((shape, out.pop(shape)))
            continue
        print(f"{shape}: " + json.dumps({k: round(v, 3) for k, v in out[shape].items() if k.endswith("_ms")}), flush=True)
    os.remove(tmp)
    if a.ab:  # the rounds alone, into the file as it stands
        import ab_rounds
        with open(OUT) as f:
            out = json.load(f)
        for shape, got in rounds:
            ab_rounds.append(out, a.ab, shape, got["figures"], got["library"])
            print(f"{shape} [{a.ab}]: " + json.dumps({k: round(v[0], 3) for k, v in got["figures"].items()}), flush=True)
    if not a.no_write:
        with open(OUT, "w") as f:
            json.dump(out, f, indent=1)
        print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
