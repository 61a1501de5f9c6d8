"""Shared-coupling CSR batches (sga_set_csr_shared: one set of CSR rows, M field vectors): kernel time per sweep and
coupling bytes held against what the parent commit offers for the same work -- sga_set_csr_batch on the rows written M
times -- and the one-model C3 line through the parent commit's library and through this build.  Written to
profiles/shared_csr.json.

Batches, M = 32 field vectors x 32 replicas (h in {-1, 0, 1}, differing per model; one 3 -> 0.3 ladder per model, no
exchange), both engines in ONE process:
  lattice   3-D +-J lattice, n = 22^3 = 10 648, degree 6
  c3        C3's graph: 10 000 spins, degree ~32, +-1 couplings
  (i)  ragged   sga_set_csr_batch on the tiled CSR: the narrow one-update int8 form
  (ii) shared   sga_set_csr_shared: the form one model would run
Final spins and energies of (i) and (ii) must be equal: asserted.  Coupling bytes = device memory the process holds
once the problem is set (the caller's arrays are host memory), against before.
One model, C3 (4096 replicas, ladder 3 -> 0.3): `--reps` (5) runs through `--baseline` (libsga.so of the parent commit:
profiles/build_variant.sh in a checkout of it; loaded through SGA_LIBRARY_PATH) alternating with as many through this
build, each in a process of its own.  The kernels of a one-model launch gained a run-time base for h; the condition on it:
this build's median lies within the min-max spread of the parent's runs.  Both series are written out.
Kernel time is the engine's own (events around every sweep launch) over `--sweeps` sweeps after `--warmup`.
usage: shared_csr_timing.py --baseline <libsga.so of the parent commit> [--reps 5] [--no-write]"""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "shared_csr.json")
M, K = 32, 32


def lattice3d(L, seed):
    rng = np.random.RandomState(seed)
    idx = np.arange(L ** 3).reshape(L, L, L)
    rows, cols, vals = [], [], []
    for ax in range(3):
        nb = np.roll(idx, -1, axis=ax)
        v = rng.randint(0, 2, idx.size) * 2.0 - 1.0
        rows += [idx.ravel(), nb.ravel()]
        cols += [nb.ravel(), idx.ravel()]
        vals += [v, v]
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(L ** 3,) * 2).tocsr()
    A.sort_indices()
    return A


def random_graph(n, half_degree, seed):
    rng = np.random.RandomState(seed)
    rows = np.repeat(np.arange(n), half_degree)
    cols = rng.randint(0, n, rows.size)
    keep = rows != cols
    lo, hi = np.minimum(rows[keep], cols[keep]), np.maximum(rows[keep], cols[keep])
    up = sp.coo_matrix((np.ones(lo.size), (lo, hi)), shape=(n, n)).tocsr()
    up.data[:] = rng.randint(0, 2, up.nnz) * 2.0 - 1.0
    A = (up + up.T).tocsr()
    A.sort_indices()
    return A


def csr(A):
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float32)


CASES = {"lattice": lambda: lattice3d(22, 1), "c3": lambda: random_graph(10000, 16, 3)}


def bind_what_the_library_has(N):
    if os.environ.get("SGA_LIBRARY_PATH"):  # an older library: bind what it has (the one-model line calls nothing newer)
        have = ctypes.CDLL(N.library_path())
        N.SYMBOLS[:] = [s for s in N.SYMBOLS if hasattr(have, s[0])]


def timed(e, n, R, warmup, sweeps):
    e.enable_timing(True)
    e.sweep(warmup)
    e.kernel_time(reset=True)
    acc0 = e.stats()[0].copy()
    e.sweep(sweeps)
    launches, ms = e.kernel_time(reset=True)
    d = (e.stats()[0] - acc0).astype(np.float64)
    return {"kernel_ms_per_sweep": ms / sweeps, "launches": launches, "sweeps": sweeps, "warmup": warmup,
            "acceptance_rate": float(d.sum()) / (float(R) * n * sweeps), "kernel": e.last_kernel(), "describe": e.describe()}


def batches(warmup, sweeps):
    """(i) and (ii) for both graphs, one process."""
    import torch
    import spin_glass_anneal_rl_amd as sg
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    out = {}
    for name, make in CASES.items():
        rp, ci, v = csr(make())
        n, R = len(rp) - 1, M * K
        H = np.random.RandomState(5).randint(-1, 2, (M, n)).astype(np.float32)
        temps = np.tile(np.geomspace(3.0, 0.3, K), M)
        entry = {"n": n, "nnz": int(len(ci)), "longest_row": int(np.diff(rp).max()), "models": M, "replicas_per_model": K}
        final = {}
        for how in ("ragged", "shared"):
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            with sg.AnnealEngine(0) as e:
                if how == "ragged":
                    e.set_csr_batch([(rp, ci, v, h) for h in H])
                else:
                    e.set_csr_shared(rp, ci, v, H)
                torch.cuda.synchronize()
                held = free0 - torch.cuda.mem_get_info()[0]
                e.init_replicas(R, seed=42)
                e.set_ladder(temps, n_ladders=M)
                entry[how] = timed(e, n, R, warmup, sweeps)
                entry[how]["coupling_bytes_held"] = int(held)
                final[how] = (hashlib.sha256(np.ascontiguousarray(e.spins()).tobytes()).hexdigest(), e.energies().tolist())
        assert final["ragged"] == final["shared"], f"{name}: the two engines' final spins / energies differ"
        entry["final_spins_and_energies_equal"] = True
        entry["ragged_over_shared"] = {"kernel_time": entry["ragged"]["kernel_ms_per_sweep"] / entry["shared"]["kernel_ms_per_sweep"],
                                       "coupling_bytes": entry["ragged"]["coupling_bytes_held"] / max(entry["shared"]["coupling_bytes_held"], 1)}
        out[name] = entry
    return out


def one_model(warmup, sweeps):
    """The one-model C3 line with whatever library SGA_LIBRARY_PATH names."""
    from spin_glass_anneal_rl_amd import _native as N
    bind_what_the_library_has(N)
    import spin_glass_anneal_rl_amd as sg
    rp, ci, v = csr(CASES["c3"]())
    n, R = len(rp) - 1, 4096
    with sg.AnnealEngine(0) as e:
        e.set_csr(rp, ci, v, np.zeros(n, np.float32))
        e.init_replicas(R, seed=11)
        e.set_ladder(np.geomspace(3.0, 0.3, R))
        res = timed(e, n, R, warmup, sweeps)
        res["final_spins_sha256"] = hashlib.sha256(np.ascontiguousarray(e.spins()).tobytes()).hexdigest()
    res.update(library=N.library_path(), version=N.lib().sga_version())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="libsga.so of the parent commit (profiles/build_variant.sh in a checkout of it)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--worker", choices=["one_model"])
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        with open(a.out, "w") as f:
            json.dump(one_model(a.warmup, a.sweeps), f)
        return
    if not a.baseline or not os.path.exists(a.baseline):
        sys.exit("--baseline <library of the parent commit> is required")
    out = {"note": "kernel ms per sweep from the engine's events; coupling_bytes_held = device memory the process holds once "
                   "the problem is set, against before (layout entries, extents, fields)"}
    out["batches"] = batches(a.warmup, a.sweeps)
    import torch
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out["batches"], indent=1), flush=True)
    fd, tmp = tempfile.mkstemp(suffix=".json")
    os.close(fd)
    runs = {"parent": [], "this_build": []}
    for rep in range(a.reps):  # alternating
        for name in runs:
            env = dict(os.environ)
            env.pop("SGA_LIBRARY_PATH", None)
            if name == "parent":
                env["SGA_LIBRARY_PATH"] = os.path.abspath(a.baseline)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "one_model", "--out", tmp, "--warmup", str(a.warmup),
                   "--sweeps", str(a.sweeps)]
            proc = subprocess.run(cmd, env=env, timeout=300)
            if proc.returncode != 0:  # (nothing more is started on the device after a failed run)
                sys.exit(f"one-model run {name} (repetition {rep}) failed with status {proc.returncode}")
            with open(tmp) as f:
                runs[name].append(json.load(f))
            print(f"rep {rep} {name}: {runs[name][-1]['kernel_ms_per_sweep']:.4f} ms per sweep", flush=True)
    os.remove(tmp)
    assert len({r["final_spins_sha256"] for rs in runs.values() for r in rs}) == 1, "one-model C3: the final spins differ"
    line = {}
    for name, rs in runs.items():
        ms = [r["kernel_ms_per_sweep"] for r in rs]
        line[name] = {"kernel_ms_per_sweep_runs": ms, "median": float(np.median(ms)), "min": min(ms), "max": max(ms),
                      "kernel": rs[0]["kernel"], "library_version": rs[0]["version"], "acceptance_rate": rs[0]["acceptance_rate"]}
    line["this_build_median_within_parent_min_max"] = bool(line["parent"]["min"] <= line["this_build"]["median"] <= line["parent"]["max"])
    line["final_spins_equal_in_every_run"] = True
    out["one_model_c3"] = line
    print(json.dumps(line, indent=1))
    if not a.no_write:
        with open(OUT, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
