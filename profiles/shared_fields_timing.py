"""Shared-coupling batches (sga_set_dense_shared: one J, M field vectors): kernel time per sweep and engine memory of
the shared engine's forms against the STACKED batch (sga_set_dense_batch on J tiled M times) on the library of the parent
commit -- built as a variant in a checkout of that commit (profiles/build_variant.sh) and loaded through
SGA_LIBRARY_PATH -- written to profiles/shared_fields.json.

Lines, +-1 couplings and h in {-1, 0, 1} differing per model, one 10 -> 0.1 ladder per model, no exchange:
  n = 10^4, M = 32 field vectors x 32 replicas         n = 1024, M = 32 x 8
Cells (each in a process of its own: a library is loaded once per process):
  shared_row_shared   row-shared windows forced (option "row_shared" = 1), field cache OFF
  shared_rows_i8      one row per proposal, int8 rows      (option "row_shared" = 0)
  shared_rows_t2      one row per proposal, bit-planes     (option "row_shared" = 0, storage "t2")
  shared_cached_on    cached local fields ON
  stacked_rows        parent library, sga_set_dense_batch, field cache OFF
  stacked_cached_on   parent library, sga_set_dense_batch, field cache ON
The cells ALTERNATE, `--reps` times (default 2); a cell's figure is the mean over its repetitions and the spread
(max - min) / mean is recorded beside it.  Kernel time is the engine's own (events around every sweep launch,
AnnealEngine.enable_timing / kernel_time) over `--sweeps` sweeps after `--warmup`; engine memory is the device memory
the process holds once the couplings are set, the replicas laid out and the form's scratch built (the caller's own
tensors released), against the start.  Final spins and energies must be equal in every cell of a line: asserted.
usage: shared_fields_timing.py --baseline <libsga.so of the parent commit> [--reps 2] [--quick] [--no-write]"""
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
OUT = os.path.join(ROOT, "profiles", "shared_fields.json")

CELLS = {  # name: (stacked, field cache, storage, options)
    "shared_row_shared": (False, "off", "auto", {"row_shared": 1}),
    "shared_rows_i8": (False, "off", "i8", {"row_shared": 0}),
    "shared_rows_t2": (False, "off", "t2", {"row_shared": 0}),
    "shared_cached_on": (False, "on", "auto", {}),
    "stacked_rows": (True, "off", "auto", {}),
    "stacked_cached_on": (True, "on", "auto", {}),
}
LINES = [(10000, 32, 32), (1024, 32, 8)]  # (n, M, k)


def ladder(k, tmax, tmin):
    return np.asarray([tmax * (tmin / tmax) ** (i / max(k - 1, 1)) for i in range(k)])


def problem(torch, n, M, seed):
    g = torch.Generator("cuda").manual_seed(seed)
    U = torch.triu((torch.randint(0, 2, (n, n), device="cuda", generator=g) * 2 - 1).float(), 1)
    return U + U.T, torch.randint(-1, 2, (M, n), device="cuda", generator=g).float()


def worker(cell, quick, warmup, sweeps):
    import torch
    from spin_glass_anneal_rl_amd import _native as N
    if os.environ.get("SGA_LIBRARY_PATH"):  # an older library: bind what it has (the stacked cells call nothing newer)
        have = ctypes.CDLL(N.library_path())
        N.SYMBOLS[:] = [s for s in N.SYMBOLS if hasattr(have, s[0])]
    import spin_glass_anneal_rl_amd as sg
    stacked, cache, storage, options = CELLS[cell]
    out = {"library": N.library_path(), "version": N.lib().sga_version(), "cell": cell}
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    for n, M, k in (LINES[1:] if quick else LINES):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free0 = torch.cuda.mem_get_info()[0]
        J, H = problem(torch, n, M, 7 + n)
        R = M * k
        with sg.AnnealEngine(0) as e:
            e.set_options(options)
            e.set_field_cache(cache)
            if stacked:
                Js = J.unsqueeze(0).expand(M, n, n).contiguous()
                e.set_dense_batch(Js, H, storage=storage)
                del Js
            else:
                e.set_dense_shared(J, H, storage=storage)
            del J, H
            e.init_replicas(R, seed=42)
            e.set_ladder(np.tile(ladder(k, 10.0, 0.1), M), n_ladders=M)
            e.enable_timing(True)
            e.sweep(warmup)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            held = free0 - torch.cuda.mem_get_info()[0]
            e.kernel_time(reset=True)
            acc0 = e.stats()[0].copy()
            e.sweep(sweeps)
            launches, ms = e.kernel_time(reset=True)
            d = (e.stats()[0] - acc0).astype(np.float64)
            spins, energies = e.spins(), e.energies()
            out[f"n{n}_M{M}_k{k}"] = {
                "kernel_ms_per_sweep": ms / sweeps, "launches": launches, "sweeps": sweeps, "warmup": warmup,
                "engine_bytes": int(held), "acceptance_rate": float(d.sum()) / (float(R) * n * sweeps),
                "kernel": e.last_kernel(), "describe": e.describe(),
                "final_spins_sha256": hashlib.sha256(np.ascontiguousarray(spins).tobytes()).hexdigest(),
                "final_energies": energies.tolist()}
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="libsga.so of the parent commit (profiles/build_variant.sh in a checkout of it)")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="the n = 1024 line only")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--worker", help="run one cell with the library loaded and write its lines")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        res = worker(a.worker, a.quick, a.warmup, a.sweeps)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f)
        else:
            print(json.dumps(res, indent=1))
        return
    if not a.baseline or not os.path.exists(a.baseline):
        sys.exit("--baseline <library of the parent commit> is required")
    runs = {c: [] for c in CELLS}
    fd, tmp = tempfile.mkstemp(suffix=".json")
    os.close(fd)
    for rep in range(a.reps):  # alternating: every cell once, then every cell again
        for name in CELLS:
            env = dict(os.environ)
            env.pop("SGA_LIBRARY_PATH", None)
            if CELLS[name][0]:
                env["SGA_LIBRARY_PATH"] = os.path.abspath(a.baseline)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", name, "--out", tmp, "--warmup", str(a.warmup),
                   "--sweeps", str(a.sweeps)] + (["--quick"] if a.quick else [])
            proc = subprocess.run(cmd, env=env, timeout=600)
            if proc.returncode != 0:  # (nothing more is started on the device after a failed cell)
                sys.exit(f"cell {name} (repetition {rep}) failed with status {proc.returncode}")
            with open(tmp) as f:
                runs[name].append(json.load(f))
            print(f"rep {rep} {name} done", flush=True)
    os.remove(tmp)
    import torch
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
           "note": "kernel ms per sweep from the engine's events; mean over the alternating repetitions, spread = (max - min) "
                   "/ mean; engine_bytes = device memory held by the process beyond its start, couplings set, replicas laid "
                   "out, the form's scratch built"}
    for line in [k for k in runs["shared_rows_i8"][0] if k.startswith("n")]:
        entry, ref = {}, None
        for name in CELLS:
            cells = [r[line] for r in runs[name]]
            ms = [c["kernel_ms_per_sweep"] for c in cells]
            for c in cells:  # the same chain in every cell, bit for bit
                ref = ref or c
                assert c["final_spins_sha256"] == ref["final_spins_sha256"], f"final spins differ: {line} {name}"
                assert c["final_energies"] == ref["final_energies"], f"final energies differ: {line} {name}"
            entry[name] = {"kernel_ms_per_sweep": float(np.mean(ms)), "kernel_ms_per_sweep_runs": ms,
                           "spread": float((max(ms) - min(ms)) / np.mean(ms)), "engine_bytes": cells[0]["engine_bytes"],
                           "acceptance_rate": cells[0]["acceptance_rate"], "kernel": cells[0]["kernel"],
                           "describe": cells[0]["describe"], "library_version": runs[name][0]["version"]}
        entry["final_spins_and_energies_equal_in_every_cell"] = True
        entry["final_energies_checksum"] = float(np.sum(ref["final_energies"]))
        base = entry["stacked_rows"]["kernel_ms_per_sweep"]
        entry["stacked_rows_over"] = {c: base / entry[c]["kernel_ms_per_sweep"] for c in CELLS if c != "stacked_rows"}
        out[line] = entry
    print(json.dumps(out, indent=1))
    if not a.no_write:
        with open(OUT, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
