"""The tile kernel's plan (csrc/sweep_dense_rs.hip, rs_tile_plan_kernel) against the parent commit's library: what
profiles/tile_plan.json and profiles/tile_plan_kernel_stats.csv hold.

  --baseline LIB   libsga.so of the parent commit (every part runs both libraries; SGA_LIBRARY_PATH selects)
  --parts a,b,...  stats    kernel time per sweep by part (plan | fields | chain | other), one `rocprofv3 --kernel-trace
                            --stats` run of 25 sweeps per cell and library: C2a at forced W = 256 / 512 / 1024, 64 and 8
                            replicas at W = 1024, 8 at W = 256, and the non-default tile cells of tiled_fields_timing.py (n = 2000, the
                            general planes), tiles forced
                   pmc      SQ_INSTS_VALU, SQ_INSTS_LDS, SQ_WAVE_CYCLES and WRITE_SIZE per sweep of the plan and tile
                            kernels, C2a at W = 1024; `rocprofv3 --pmc` runs of their own, no tracing beside them
                   ab       alternating plain runs of `bench.py --gpus 1 --steps 20 --warmup 5`, --runs of each library,
                            and --dump-outputs of both compared array for array
                   other    bench.py --workload c3 | c4 | c5, three alternating runs of each library
                   tune     sga_autotune on the C2a instance: wall time, its row-shared table, its pick
  --variants n=LIB,...  further libraries (throwaway builds: the neighbours of rg, the other ways to load a tile's rows) for
                        the stats cells of --variant-cells and the plain runs

usage: tile_plan_timing.py --baseline LIB [--parts ...] [--runs 4] [--variants rg8=build/libsga_rg8.so,...]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "tile_plan.json")
OUT_CSV = os.path.join(ROOT, "profiles", "tile_plan_kernel_stats.csv")
BENCH = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"]
TILED = os.path.join(ROOT, "profiles", "tiled_fields_timing.py")
SWEEPS = 25
PLAN = ("rs_plan_kernel", "rs_scan", "rs_tile_plan_kernel")


def part_of(short):
    return ("fields" if short.startswith("rs_fields") else "chain" if short.startswith("rs_chain") else
            "planes (once)" if short.startswith("rs_planes") else "plan" if short.startswith(PLAN) else "other")


def env_of(lib, **add):
    env = dict(os.environ, **{k: str(v) for k, v in add.items()})
    env.pop("SGA_LIBRARY_PATH", None)
    if lib:
        env["SGA_LIBRARY_PATH"] = os.path.abspath(lib)
    return env


def last_json(text):
    return json.loads(next(ln for ln in text.splitlines()[::-1] if ln.startswith("{")))


def stats_cells():
    c = {f"c2a_W{W}": ({"SGA_ROW_SHARED_WINDOW": W}, BENCH + ["--no-autotune"]) for W in (256, 512, 1024)}
    for R in (64, 8):
        c[f"r{R}_W1024"] = ({"SGA_ROW_SHARED_WINDOW": 1024}, BENCH + ["--no-autotune", "--replicas", str(R)])
    c["r8_W256"] = ({"SGA_ROW_SHARED_WINDOW": 256}, BENCH + ["--no-autotune", "--replicas", "8"])
    c["n2000_W1024_tiles"] = ({"SGA_ROW_SHARED_WINDOW": 1024, "SGA_ROW_SHARED_FIELDS": 1}, BENCH + ["--no-autotune", "--spins", "2000"])
    for kind in ("hole", "a7", "a100"):
        c[f"gen_{kind}_tiles"] = ({"SGA_ROW_SHARED_WINDOW": 1024, "SGA_ROW_SHARED_FIELDS": 1}, [sys.executable, TILED, "--drive", kind])
    return c


def profiled(cmd, env, rocprof_args, pattern):
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3"] + rocprof_args + ["-d", d, "--output-format", "csv", "--"] + cmd, env=env, capture_output=True,
                           text=True, timeout=400)
        if p.returncode != 0:
            raise SystemExit(f"{cmd}: exit {p.returncode}\n{p.stderr[-800:]}")
        rows = list(csv.reader(open(glob.glob(os.path.join(d, "**", pattern), recursive=True)[0])))
    return last_json(p.stdout), rows


def stats_cell(env_add, cmd, lib):
    res, rows = profiled(cmd, env_of(lib, SGA_ROW_SHARED=1, **env_add), ["--kernel-trace", "--stats"], "*kernel_stats.csv")
    head, body = rows[0], [r for r in rows[1:] if "sga::rs_" in r[0] or "sga::update_best" in r[0]]
    col = {h: i for i, h in enumerate(head)}
    per_sweep, launch = {}, {}
    for r in body:
        short = r[0].split("sga::")[1].split("(")[0]
        per_sweep[part_of(short)] = per_sweep.get(part_of(short), 0.0) + float(r[col["TotalDurationNs"]]) / SWEEPS / 1e6
        if part_of(short) in ("plan", "fields"):
            launch[short] = {"calls": int(r[col["Calls"]]), "avg_us": float(r[col["AverageNs"]]) / 1e3}
    return ({"ms_per_step": res["ms_per_step"], "kernel": res["roofline"]["kernel_instantiation"],
             "ms_per_sweep": {k: round(v, 4) for k, v in sorted(per_sweep.items())}, "us_per_launch": launch}, head, body)


def pmc_cell(lib):
    """Counters summed over the 25 sweeps' dispatches of a kernel, per sweep."""
    out = {}
    for counters in (["SQ_INSTS_VALU", "SQ_INSTS_LDS", "SQ_WAVE_CYCLES"], ["WRITE_SIZE"]):
        _, rows = profiled(BENCH + ["--no-autotune"], env_of(lib, SGA_ROW_SHARED=1, SGA_ROW_SHARED_WINDOW=1024), ["--pmc"] + counters,
                           "*counter_collection.csv")
        col = {h: i for i, h in enumerate(rows[0])}
        for r in rows[1:]:
            name = r[col["Kernel_Name"]]
            if "sga::rs_" not in name:
                continue
            short = name.split("sga::")[1].split("(")[0]
            if part_of(short) in ("plan", "fields"):
                k = out.setdefault(short, {})
                k[r[col["Counter_Name"]]] = k.get(r[col["Counter_Name"]], 0.0) + float(r[col["Counter_Value"]]) / SWEEPS
    return out


def plain(lib, extra=(), dump=None):
    cmd = BENCH + list(extra) + (["--dump-outputs", dump] if dump else [])
    p = subprocess.run(cmd, env=env_of(lib), capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"{cmd}: exit {p.returncode}\n{p.stderr[-800:]}")
    return last_json(p.stdout)["ms_per_step"]


def tune():
    """C2a's instance under default options: sga_autotune's wall time, its row-shared table, its pick (one JSON line)."""
    sys.path.insert(0, ROOT)
    import spin_glass_anneal_rl_amd as sg
    n, R = 10000, 1024
    rng = np.random.RandomState(7)
    A = np.triu((rng.randint(0, 2, (n, n), dtype=np.int8) * 2 - 1).astype(np.int8), 1)
    J = (A + A.T).astype(np.float32)
    tmax = 2.0 * np.sqrt(n)
    with sg.AnnealEngine(0) as e:
        e.set_dense(J, np.zeros(n, np.float32), storage="f32")
        e.init_replicas(R, seed=11)
        e.set_ladder(np.asarray([tmax * (0.3 / tmax) ** (i / (R - 1)) for i in range(R)]))
        e.sweep(2)
        e.energies()
        t0 = time.perf_counter()
        e.autotune()
        wall = time.perf_counter() - t0
        table = {k: v for k, v in e.autotune_table(forms=True).items() if k.startswith("row-shared:")}
        e.sweep(1)
        print(json.dumps({"autotune_wall_s": round(wall, 3), "row_shared_ms_per_sweep": table, "kernel": e.last_kernel()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline")
    ap.add_argument("--parts", default="stats,pmc,ab,other,tune")
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--variants", default="")
    ap.add_argument("--variant-cells", default="c2a_W1024")
    ap.add_argument("--stats-libs", default="parent,new", help="the stats part only: which of the two libraries to run")
    ap.add_argument("--tune", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.tune:
        return tune()
    libs = {"parent": a.baseline, "new": None}
    merged = json.load(open(OUT)) if os.path.exists(OUT) else {}

    def save():
        json.dump(merged, open(OUT, "w"), indent=1)

    parts = a.parts.split(",")
    variants = dict(v.split("=") for v in a.variants.split(",") if v)
    if "stats" in parts:
        kept = [r for r in csv.reader(open(OUT_CSV))][1:] if os.path.exists(OUT_CSV) else []
        cells = [(name, lib, spec) for name, spec in stats_cells().items() for lib in a.stats_libs.split(",")]
        cells += [(name, v, stats_cells()[name]) for name in a.variant_cells.split(",") for v in variants]
        for name, lib, (env_add, cmd) in cells:
            cell, head, body = stats_cell(env_add, cmd, {**libs, **variants}[lib])
            print(name, lib, json.dumps(cell), flush=True)
            merged.setdefault("stats", {}).setdefault(name, {})[lib] = cell
            save()
            kept = [r for r in kept if r[0] != f"{name}:{lib}"] + [[f"{name}:{lib}"] + r for r in body]
            with open(OUT_CSV, "w", newline="") as f:
                csv.writer(f).writerows([["cell"] + head] + kept)
    if "pmc" in parts:
        for lib in libs:
            merged.setdefault("pmc_per_sweep_c2a_W1024", {})[lib] = pmc_cell(libs[lib])
            print("pmc", lib, json.dumps(merged["pmc_per_sweep_c2a_W1024"][lib]), flush=True)
            save()
    if "ab" in parts:
        ms = {lib: [] for lib in {**libs, **variants}}
        for _ in range(a.runs):
            for lib in ms:
                ms[lib].append(plain({**libs, **variants}[lib]))
                print("ab", lib, ms[lib][-1], flush=True)
        with tempfile.TemporaryDirectory() as d:
            for lib in libs:
                plain(libs[lib], dump=os.path.join(d, lib))
            names = sorted(os.listdir(os.path.join(d, "parent")))
            same = names == sorted(os.listdir(os.path.join(d, "new"))) and all(
                np.array_equal(np.load(os.path.join(d, "parent", f)), np.load(os.path.join(d, "new", f))) for f in names)
        spread = max(ms["parent"]) - min(ms["parent"])
        merged["ab_c2a"] = {"ms_per_step": ms, "parent_spread_ms": spread, "gain_ms_worst_case": min(ms["parent"]) - max(ms["new"]),
                            "criterion_10x_spread_met": bool(min(ms["parent"]) - max(ms["new"]) >= 10 * spread),
                            "dumped_arrays": names, "dumped_arrays_equal": bool(same)}
        print("ab", json.dumps(merged["ab_c2a"]), flush=True)
        save()
    if "other" in parts:
        for wl in ("c3", "c4", "c5"):
            ms = {lib: [] for lib in libs}
            for _ in range(3):
                for lib in libs:
                    ms[lib].append(plain(libs[lib], extra=["--workload", wl]))
            merged.setdefault("other_workloads", {})[wl] = {"ms_per_step": ms, "median": {k: float(np.median(v)) for k, v in ms.items()}}
            print(wl, json.dumps(merged["other_workloads"][wl]), flush=True)
            save()
    if "tune" in parts:
        for lib in libs:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--tune"], env=env_of(libs[lib]), capture_output=True, text=True,
                               timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"tune {lib}: exit {p.returncode}\n{p.stderr[-800:]}")
            merged.setdefault("autotune_c2a", {})[lib] = last_json(p.stdout)
            print("tune", lib, json.dumps(merged["autotune_c2a"][lib]), flush=True)
            save()


if __name__ == "__main__":
    main()
