"""Row-shared fields in tiles of sites (options "row_shared_fields", "row_shared_tile_sites"; csrc/sweep_dense_rs.hip,
rs_fields_tiles_kernel): ms per step of bench.py and kernel time per sweep of the row-shared kernels, per cell -- written to
profiles/tiled_fields.json and profiles/tiled_fields_kernel_stats.csv.

Every cell is one `rocprofv3 --kernel-trace --stats` run of `bench.py --gpus 1 --steps 20 --warmup 5 --no-autotune` (25
sweeps, the hot first ones included) with the form forced through the environment (SGA_ROW_SHARED=1,
SGA_ROW_SHARED_WINDOW=W) and the fields kernel chosen by SGA_ROW_SHARED_FIELDS / SGA_ROW_SHARED_TILE_SITES:

  c2a_W{256,512,1024}_{site,tiles}      C2a (n = 10 000, 1024 replicas), per-site kernel | tiles at the host rule's S
  c2a_W1024_S{10,20,80}                 the neighbours of the rule's S = 40
  n2000_W1024_{site,tiles,default}      n = 2000 x 1024 replicas: per-site | tiles forced (SGA_ROW_SHARED_FIELDS=1) | the
                                        default, which keeps the per-site kernel under 1 KB of spin bits per replica

  gen_{hole,a7,a100}_{site,tiles}       the general (not sign-only) planes at C2a's shape, n = 10 000 x 1024 replicas, W =
                                        1024, tiles forced (SGA_ROW_SHARED_FIELDS=1): +-1 with one pair set to 0 (one
                                        magnitude plane, the bits in registers), |J| <= 7 (three planes: at this n the
                                        bits stream per entry), fp32 |J| <= 100 (eight resident planes: they always stream)

The gen_ cells do not go through bench.py, which has no such couplings: the same rocprofv3 line runs this file with
--drive KIND, 25 single sweeps of an engine of its own.  --baseline <libsga.so of the parent commit> adds c2a_W1024_parent.  ms_per_step is the profiled run's own (tracing costs
a few per cent); the A/B of plain runs is taken without the profiler (alternating `bench.py --gpus 1 --steps 20 --warmup
5` of the two libraries through SGA_LIBRARY_PATH).

The files are rewritten after every cell; cells not run keep their entries and rows.

usage: tiled_fields_timing.py [--baseline LIB] [--cells a,b,...] [--no-write]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "tiled_fields.json")
OUT_CSV = os.path.join(ROOT, "profiles", "tiled_fields_kernel_stats.csv")
SWEEPS = 25


def cells(baseline):
    c = {}
    for W in (256, 512, 1024):
        c[f"c2a_W{W}_site"] = ({"SGA_ROW_SHARED_WINDOW": W, "SGA_ROW_SHARED_FIELDS": 0}, [], None)
        c[f"c2a_W{W}_tiles"] = ({"SGA_ROW_SHARED_WINDOW": W}, [], None)
    for S in (10, 20, 80):
        c[f"c2a_W1024_S{S}"] = ({"SGA_ROW_SHARED_WINDOW": 1024, "SGA_ROW_SHARED_TILE_SITES": S}, [], None)
    c["n2000_W1024_site"] = ({"SGA_ROW_SHARED_WINDOW": 1024, "SGA_ROW_SHARED_FIELDS": 0}, ["--spins", "2000"], None)
    c["n2000_W1024_tiles"] = ({"SGA_ROW_SHARED_WINDOW": 1024, "SGA_ROW_SHARED_FIELDS": 1}, ["--spins", "2000"], None)
    c["n2000_W1024_default"] = ({"SGA_ROW_SHARED_WINDOW": 1024}, ["--spins", "2000"], None)
    for kind in ("hole", "a7", "a100"):
        c[f"gen_{kind}_site"] = ({"SGA_ROW_SHARED_WINDOW": 1024, "SGA_ROW_SHARED_FIELDS": 0}, ["--drive", kind], None)
        c[f"gen_{kind}_tiles"] = ({"SGA_ROW_SHARED_WINDOW": 1024, "SGA_ROW_SHARED_FIELDS": 1}, ["--drive", kind], None)
    if baseline:
        c["c2a_W1024_parent"] = ({"SGA_ROW_SHARED_WINDOW": 1024}, [], os.path.abspath(baseline))
    return c


def drive(kind, n=10000, R=1024):
    """25 single sweeps of a dense problem bench.py does not have (kind: "hole" | "a7" | "a100"), the options from the
    environment; one JSON line in the shape of bench.py's as far as run_cell reads it."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import spin_glass_anneal_rl_amd as sg
    rng = np.random.RandomState(7)
    amp = {"hole": 1, "a7": 7, "a100": 100}[kind]
    A = rng.randint(0, 2, (n, n), dtype=np.int8) * 2 - 1 if kind == "hole" else rng.randint(-amp, amp + 1, (n, n), dtype=np.int8)
    A = np.triu(A.astype(np.int8), 1)
    if kind == "hole":
        A[n // 3, n - 2] = 0
    J = (A + A.T).astype(np.float32)
    h = rng.randint(-1, 2, n).astype(np.float32)
    tmax = 2.0 * amp * np.sqrt(n)
    with sg.AnnealEngine(0) as e:
        for key in ("row_shared", "row_shared_window", "row_shared_fields", "row_shared_tile_sites"):
            if "SGA_" + key.upper() in os.environ:
                e.set_option(key, int(os.environ["SGA_" + key.upper()]))
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=11)
        e.set_ladder(np.asarray([tmax * (0.3 / tmax) ** (i / (R - 1)) for i in range(R)]))
        for _ in range(5):
            e.sweep(1)
        e.energies()
        t0 = time.perf_counter()
        for _ in range(SWEEPS - 5):
            e.sweep(1)
        e.energies()
        ms = (time.perf_counter() - t0) * 1e3 / (SWEEPS - 5)
        print(json.dumps({"ms_per_step": ms, "roofline": {"kernel_instantiation": e.last_kernel()}, "describe": e.describe()}))


def run_cell(name, env_add, args, lib):
    env = dict(os.environ, SGA_ROW_SHARED="1", **{k: str(v) for k, v in env_add.items()})
    if lib:
        env["SGA_LIBRARY_PATH"] = lib
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable]
        if args[:1] == ["--drive"]:
            cmd += [os.path.abspath(__file__)] + args
        else:
            cmd += [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-autotune"] + args
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            raise SystemExit(f"{name}: exit {p.returncode}\n{p.stderr[-800:]}")
        line = next(ln for ln in p.stdout.splitlines()[::-1] if ln.startswith("{"))
        res = json.loads(line)
        rows = list(csv.reader(open(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0])))
    head, body = rows[0], [r for r in rows[1:] if "sga::rs_" in r[0] or "sga::update_best" in r[0]]
    col = {h: i for i, h in enumerate(head)}
    per_sweep = {}
    for r in body:
        short = r[0].split("sga::")[1].split("(")[0]
        part = ("fields" if short.startswith("rs_fields") else "chain" if short.startswith("rs_chain") else
                "planes (once)" if short.startswith("rs_planes") else "plan" if short.startswith(("rs_plan", "rs_scan")) else "other")
        per_sweep[part] = per_sweep.get(part, 0.0) + float(r[col["TotalDurationNs"]]) / SWEEPS / 1e6
    fields = [r for r in body if "rs_fields" in r[0]]
    out = {"ms_per_step": res["ms_per_step"], "kernel": res["roofline"]["kernel_instantiation"],
           "ms_per_sweep": {k: round(v, 4) for k, v in sorted(per_sweep.items())},
           "fields_us_per_launch": {k: float(fields[0][col[c]]) / 1e3 for k, c in
                                    (("avg", "AverageNs"), ("min", "MinNs"), ("max", "MaxNs"))} if fields else None}
    return out, head, body


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline")
    ap.add_argument("--cells")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--drive", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.drive:
        return drive(a.drive)
    todo = cells(a.baseline)
    if a.cells:
        todo = {k: todo[k] for k in a.cells.split(",")}
    for name, (env_add, args, lib) in todo.items():
        cell, head, body = run_cell(name, env_add, args, lib)
        print(name, json.dumps(cell), flush=True)
        if a.no_write:
            continue
        merged = json.load(open(OUT)) if os.path.exists(OUT) else {}
        merged.setdefault("cells", {})[name] = cell
        json.dump(merged, open(OUT, "w"), indent=1)
        kept = [r for r in csv.reader(open(OUT_CSV))][1:] if os.path.exists(OUT_CSV) else []
        with open(OUT_CSV, "w", newline="") as f:
            csv.writer(f).writerows([["cell"] + head] + [r for r in kept if r[0] != name] + [[name] + r for r in body])


if __name__ == "__main__":
    main()
