"""Row-shared windows on a binary grid (option "row_shared_grid", csrc/sweep_dense_rs.hip GRID): kernel time per sweep
of the grid form against the row-per-proposal kernel the same problems run today, and the unchanged integer line of the
windows on this library against the parent commit's -- written to profiles/row_shared_grid.json.

Problem: n = 10^4, 1024 replicas, one ladder 10 -> 0.1 (bench.py's), field cache off, fp32 rows, random spins.
  quarter   J = +-1/4 (the SK instance of the headline as IsingBuilder.add_qubo_pair stores it), h quarter-valued
  real_h    the headline's +-1 J under a real-valued h (randn)
Forms (each cell in a process of its own):
  grid_W256 | grid_W512 | grid_W1024   the grid form forced (options "row_shared" = 1, "row_shared_grid" = 1, W)
  grid_autotune                        "row_shared" = 2, "row_shared_grid" = 1, sga_autotune after the warm-up sweeps
  rows                                 the row-per-proposal kernel ("row_shared_grid" = 0)
The cells ALTERNATE, `--reps` times (default 2); kernel time is the engine's own (events around every sweep launch) over
sweeps `--warmup` .. `--warmup` + `--sweeps` (5 .. 25) from random spins.  A cell's figure is the mean over its
repetitions, the spread (max - min) / mean beside it, with the acceptance per proposal over the timed sweeps.  Final
spins and energies must be equal in every cell of an instance: asserted.
The C2a line (integer: +-1 J, h = 0, "row_shared" = 1, W = 1024) runs the non-GRID instantiations: `--c2a-reps` runs
(default 5) on this library alternate with as many on the parent's (--baseline, loaded through SGA_LIBRARY_PATH;
profiles/build_variant.sh in a checkout of the parent builds it).  The new median must lie inside the parent's own
min .. max: asserted.
usage: row_shared_grid_timing.py --baseline <libsga.so of the parent commit> [--reps 2] [--c2a-reps 5] [--quick] [--no-write]"""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "row_shared_grid.json")

FORMS = {  # name: (options, autotune)
    "grid_W256": ({"row_shared": 1, "row_shared_grid": 1, "row_shared_window": 256}, False),
    "grid_W512": ({"row_shared": 1, "row_shared_grid": 1, "row_shared_window": 512}, False),
    "grid_W1024": ({"row_shared": 1, "row_shared_grid": 1, "row_shared_window": 1024}, False),
    "grid_autotune": ({"row_shared": 2, "row_shared_grid": 1}, True),
    "rows": ({"row_shared": 1, "row_shared_grid": 0}, False),
}
INSTANCES = ("quarter", "real_h")
C2A = ({"row_shared": 1, "row_shared_window": 1024}, False)


def ladder(k, tmax, tmin):
    return np.asarray([tmax * (tmin / tmax) ** (i / max(k - 1, 1)) for i in range(k)])


def problem(torch, instance, n):
    g = torch.Generator("cuda").manual_seed(2)
    U = torch.triu((torch.randint(0, 2, (n, n), device="cuda", generator=g, dtype=torch.int8) * 2 - 1), 1)
    J = (U + U.T).to(torch.float32)
    if instance == "quarter":  # (add_qubo_pair with q = +-1 per pair stores J = -q / 4; h on the same grid)
        return J * 0.25, torch.randint(-8, 9, (n,), device="cuda", generator=g).float() * 0.25
    if instance == "real_h":
        return J, torch.randn(n, device="cuda", generator=g)
    return J, torch.zeros(n, device="cuda")  # c2a


def worker(instance, form, n, R, warmup, sweeps):
    import torch
    from spin_glass_anneal_rl_amd import _native as N
    if os.environ.get("SGA_LIBRARY_PATH"):  # an older library: bind what it has
        have = ctypes.CDLL(N.library_path())
        N.SYMBOLS[:] = [s for s in N.SYMBOLS if hasattr(have, s[0])]
    import spin_glass_anneal_rl_amd as sg
    options, tune = C2A if instance == "c2a" else FORMS[form]
    torch.zeros(1, device="cuda")
    J, h = problem(torch, instance, n)
    with sg.AnnealEngine(0) as e:
        e.set_options(options)
        e.set_field_cache("off")
        e.set_dense(J, h, storage="f32")
        del J
        e.init_replicas(R, seed=42)
        e.set_ladder(ladder(R, 10.0, 0.1))
        e.enable_timing(True)
        e.sweep(warmup)
        table = None
        if tune:
            e.autotune()
            table = e.autotune_table(forms=True)
        e.kernel_time(reset=True)
        acc0 = e.stats()[0].copy()
        e.sweep(sweeps)
        launches, ms = e.kernel_time(reset=True)
        d = (e.stats()[0] - acc0).astype(np.float64)
        spins, energies = e.spins(), e.energies()
        return {"library": N.library_path(), "version": N.lib().sga_version(), "instance": instance, "form": form,
                "kernel_ms_per_sweep": ms / sweeps, "launches": launches, "sweeps": sweeps, "warmup": warmup,
                "acceptance_per_proposal": float(d.sum()) / (float(R) * n * sweeps), "kernel": e.last_kernel(),
                "describe": e.describe(), "autotune_table": table,
                "final_spins_sha256": hashlib.sha256(np.ascontiguousarray(spins).tobytes()).hexdigest(),
                "final_energies_sha256": hashlib.sha256(np.ascontiguousarray(energies).tobytes()).hexdigest(),
                "final_energy_min": float(energies.min())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="libsga.so of the parent commit")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--c2a-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="n = 2048, 128 replicas")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--worker", nargs=2, metavar=("INSTANCE", "FORM"))
    ap.add_argument("--out")
    a = ap.parse_args()
    n, R = (2048, 128) if a.quick else (10000, 1024)
    if a.worker:
        res = worker(a.worker[0], a.worker[1], n, R, a.warmup, a.sweeps)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f)
        else:
            print(json.dumps(res, indent=1))
        return
    if not a.baseline or not os.path.exists(a.baseline):
        sys.exit("--baseline <library of the parent commit> is required")
    fd, tmp = tempfile.mkstemp(suffix=".json")
    os.close(fd)

    def cell(instance, form, library=None):
        env = dict(os.environ)
        env.pop("SGA_LIBRARY_PATH", None)
        if library:
            env["SGA_LIBRARY_PATH"] = os.path.abspath(library)
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", instance, form, "--out", tmp, "--warmup", str(a.warmup),
               "--sweeps", str(a.sweeps)] + (["--quick"] if a.quick else [])
        proc = subprocess.run(cmd, env=env, timeout=600)
        if proc.returncode != 0:  # (nothing more is started on the device after a failed cell)
            sys.exit(f"cell {instance} {form} failed with status {proc.returncode}")
        with open(tmp) as f:
            res = json.load(f)
        print(f"{instance} {form} {'parent' if library else 'this'}: {res['kernel_ms_per_sweep']:.3f} ms  {res['kernel'][:60]}", flush=True)
        return res

    # the unchanged integer line first: this library and the parent's, alternating
    new, old = [], []
    for rep in range(a.c2a_reps):  # (which library goes first alternates too)
        for parent in ((False, True) if rep % 2 == 0 else (True, False)):
            (old if parent else new).append(cell("c2a", "row_shared_W1024", a.baseline if parent else None))
    runs = {i: {f: [] for f in FORMS} for i in INSTANCES}
    for _ in range(a.reps):  # alternating: every cell once, then every cell again
        for i in INSTANCES:
            for f in FORMS:
                runs[i][f].append(cell(i, f))
    os.remove(tmp)
    import torch
    out = {"device": torch.cuda.get_device_name(0), "n": n, "replicas": R, "reps": a.reps, "sweeps_timed": [a.warmup, a.warmup + a.sweeps],
           "note": "kernel ms per sweep from the engine's events; mean over the alternating repetitions, spread = (max - min) / mean"}
    for i in INSTANCES:
        entry, ref = {}, None
        for f in FORMS:
            cells = runs[i][f]
            ms = [c["kernel_ms_per_sweep"] for c in cells]
            for c in cells:  # the same chain in every cell, bit for bit
                ref = ref or c
                assert c["final_spins_sha256"] == ref["final_spins_sha256"], f"final spins differ: {i} {f}"
                assert c["final_energies_sha256"] == ref["final_energies_sha256"], f"final energies differ: {i} {f}"
            entry[f] = {"kernel_ms_per_sweep": float(np.mean(ms)), "kernel_ms_per_sweep_runs": ms,
                        "spread": float((max(ms) - min(ms)) / np.mean(ms)), "acceptance_per_proposal": cells[0]["acceptance_per_proposal"],
                        "kernel": cells[0]["kernel"], "describe": cells[0]["describe"], "autotune_table": cells[0]["autotune_table"]}
        entry["final_spins_and_energies_equal_in_every_cell"] = True
        entry["final_energy_min"] = ref["final_energy_min"]
        rows = entry["rows"]["kernel_ms_per_sweep"]
        entry["rows_over"] = {f: rows / entry[f]["kernel_ms_per_sweep"] for f in FORMS if f != "rows"}
        out[i] = entry
    for c in new + old:
        assert c["final_spins_sha256"] == new[0]["final_spins_sha256"] and c["final_energies_sha256"] == new[0]["final_energies_sha256"]
    new_ms, old_ms = [c["kernel_ms_per_sweep"] for c in new], [c["kernel_ms_per_sweep"] for c in old]
    inside = min(old_ms) <= float(np.median(new_ms)) <= max(old_ms)
    out["c2a_integer_line_unchanged"] = {
        "kernel": new[0]["kernel"], "parent_kernel": old[0]["kernel"], "parent_version": old[0]["version"], "version": new[0]["version"],
        "kernel_ms_per_sweep_runs": new_ms, "parent_kernel_ms_per_sweep_runs": old_ms, "median": float(np.median(new_ms)),
        "parent_min": min(old_ms), "parent_max": max(old_ms), "median_inside_parent_min_max": inside,
        "final_spins_and_energies_equal": True}
    print(json.dumps(out, indent=1))
    if not a.no_write:
        with open(OUT, "w") as f:
            json.dump(out, f, indent=1)
    assert inside, ("the integer line's median left the parent's own min .. max", new_ms, old_ms)


if __name__ == "__main__":
    main()
