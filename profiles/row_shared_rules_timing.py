"""Row-shared windows under the Glauber and heat-bath rules (csrc/sweep_dense_rs.hip, ANYRULE): kernel time per sweep
of the windows against the row-per-proposal kernel those rules ran before, what sga_autotune picks under option
"row_shared" = 2, and the unchanged Metropolis line on this library against the parent commit's -- written to
profiles/row_shared_rules.json.

Problem: n = 10^4, 1024 replicas, one ladder 10 -> 0.1 (bench.py's C2a ladder), field cache off, random spins.
  integer   J = +-1, h in {-1, 0, 1}; storage is what SGA_J_AUTO picks
  quarter   J = +-1/4, h quarter-valued, option "row_shared_grid" = 1 (the grid form)
Rules: glauber, heat-bath.  Forms, each on a fresh engine (one process per instance and rule):
  rows                          option "row_shared" = 0: one coupling row per proposal
  W256 | W512 | W1024           "row_shared" = 1 at that window
  autotune                      "row_shared" = 2 and sga_autotune after the untimed sweeps: its pick and its table
Every form runs `--warmup` untimed sweeps (16, the autotuner's burn-in) and then `--sweeps` timed ones; kernel time is
the engine's own (events around every sweep launch).  Final spins and energies must be equal in every form of an
instance and rule: asserted.
The Metropolis line (integer instance, "row_shared" = 1, W = 1024) runs the instantiations this change must leave as
they were: `--metropolis-reps` runs (3) on this library alternate with as many on the parent's (--baseline, built with
profiles/build_variant.sh in a checkout of the parent and loaded through SGA_LIBRARY_PATH).  The new median must lie
inside the parent's own min .. max or no more than 1 % outside it (sga_autotune's tie margin): asserted.
usage: row_shared_rules_timing.py --baseline <libsga.so of the parent commit> [--quick] [--no-write]"""
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
OUT = os.path.join(ROOT, "profiles", "row_shared_rules.json")

FORMS = {  # name: (options, autotune)
    "rows": ({"row_shared": 0}, False),
    "W256": ({"row_shared": 1, "row_shared_window": 256}, False),
    "W512": ({"row_shared": 1, "row_shared_window": 512}, False),
    "W1024": ({"row_shared": 1, "row_shared_window": 1024}, False),
    "autotune": ({"row_shared": 2}, True),
}
INSTANCES = ("integer", "quarter")
RULES = {"metropolis": 0, "glauber": 1, "heat-bath": 2}
TIE = 0.01  # sga_autotune's tie margin


def ladder(k, tmax, tmin):
    return np.asarray([tmax * (tmin / tmax) ** (i / max(k - 1, 1)) for i in range(k)])


def problem(torch, instance, n):
    g = torch.Generator("cuda").manual_seed(2)
    U = torch.triu((torch.randint(0, 2, (n, n), device="cuda", generator=g, dtype=torch.int8) * 2 - 1), 1)
    J = (U + U.T).to(torch.float32)
    if instance == "quarter":
        return J * 0.25, torch.randint(-8, 9, (n,), device="cuda", generator=g).float() * 0.25
    return J, torch.randint(-1, 2, (n,), device="cuda", generator=g).float()


def worker(instance, rule, forms, n, R, warmup, sweeps):
    import torch
    from spin_glass_anneal_rl_amd import _native as N
    if os.environ.get("SGA_LIBRARY_PATH"):  # an older library: bind what it has
        have = ctypes.CDLL(N.library_path())
        N.SYMBOLS[:] = [s for s in N.SYMBOLS if hasattr(have, s[0])]
    import spin_glass_anneal_rl_amd as sg
    torch.zeros(1, device="cuda")
    J, h = problem(torch, instance, n)
    out = {}
    for form in forms:
        options, tune = FORMS[form]
        with sg.AnnealEngine(0) as e:
            e.set_options({**options, "row_shared_grid": 1 if instance == "quarter" else 0})
            e.set_field_cache("off")
            e.set_dense(J, h, storage="auto")
            e.set_update_rule(RULES[rule])
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
            out[form] = {"library": N.library_path(), "version": N.lib().sga_version(), "instance": instance, "rule": rule,
                         "kernel_ms_per_sweep": ms / sweeps, "launches": launches, "sweeps": sweeps, "warmup": warmup,
                         "flips_per_proposal": float(d.sum()) / (float(R) * n * sweeps), "kernel": e.last_kernel(),
                         "describe": e.describe(), "autotune_table": table,
                         "final_spins_sha256": hashlib.sha256(np.ascontiguousarray(spins).tobytes()).hexdigest(),
                         "final_energies_sha256": hashlib.sha256(np.ascontiguousarray(energies).tobytes()).hexdigest(),
                         "final_energy_min": float(energies.min())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="libsga.so of the parent commit")
    ap.add_argument("--metropolis-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="n = 2048, 128 replicas")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--worker", nargs=3, metavar=("INSTANCE", "RULE", "FORMS"))
    ap.add_argument("--out")
    a = ap.parse_args()
    n, R = (2048, 128) if a.quick else (10000, 1024)
    if a.worker:
        res = worker(a.worker[0], a.worker[1], a.worker[2].split(","), n, R, a.warmup, a.sweeps)
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

    def cell(instance, rule, forms, library=None):
        env = dict(os.environ)
        env.pop("SGA_LIBRARY_PATH", None)
        if library:
            env["SGA_LIBRARY_PATH"] = os.path.abspath(library)
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", instance, rule, ",".join(forms), "--out", tmp,
               "--warmup", str(a.warmup), "--sweeps", str(a.sweeps)] + (["--quick"] if a.quick else [])
        proc = subprocess.run(cmd, env=env, timeout=900)
        if proc.returncode != 0:  # (nothing more is started on the device after a failed cell)
            sys.exit(f"cell {instance} {rule} failed with status {proc.returncode}")
        with open(tmp) as f:
            res = json.load(f)
        for form, r in res.items():
            print(f"{instance} {rule} {form} {'parent' if library else 'this'}: {r['kernel_ms_per_sweep']:.3f} ms  {r['kernel'][:70]}",
                  flush=True)
        return res

    # the unchanged Metropolis line first: this library and the parent's, alternating
    new, old = [], []
    for rep in range(a.metropolis_reps):  # (which library goes first alternates too)
        for parent in ((False, True) if rep % 2 == 0 else (True, False)):
            (old if parent else new).append(cell("integer", "metropolis", ["W1024"], a.baseline if parent else None)["W1024"])
    import torch
    out = {"device": torch.cuda.get_device_name(0), "n": n, "replicas": R, "sweeps_timed": [a.warmup, a.warmup + a.sweeps],
           "note": "kernel ms per sweep from the engine's events over the timed sweeps, one run per form; flips_per_proposal over "
                   "the same sweeps"}
    for i in INSTANCES:
        for rule in ("glauber", "heat-bath"):
            res = cell(i, rule, list(FORMS))
            ref = res["rows"]
            entry = {}
            for f, c in res.items():  # the same chain in every form, bit for bit
                assert c["final_spins_sha256"] == ref["final_spins_sha256"], f"final spins differ: {i} {rule} {f}"
                assert c["final_energies_sha256"] == ref["final_energies_sha256"], f"final energies differ: {i} {rule} {f}"
                entry[f] = {k: c[k] for k in ("kernel_ms_per_sweep", "flips_per_proposal", "kernel", "describe", "autotune_table")}
            entry["final_spins_and_energies_equal_in_every_form"] = True
            entry["final_energy_min"] = ref["final_energy_min"]
            rows = entry["rows"]["kernel_ms_per_sweep"]
            entry["rows_over"] = {f: rows / entry[f]["kernel_ms_per_sweep"] for f in FORMS if f != "rows"}
            entry["autotune_picked"] = entry["autotune"]["kernel"].split(" (")[0]
            out[f"{i}_{rule}"] = entry
    os.remove(tmp)
    for c in new + old:
        assert c["final_spins_sha256"] == new[0]["final_spins_sha256"] and c["final_energies_sha256"] == new[0]["final_energies_sha256"]
    new_ms, old_ms = [c["kernel_ms_per_sweep"] for c in new], [c["kernel_ms_per_sweep"] for c in old]
    med = float(np.median(new_ms))
    inside = min(old_ms) * (1.0 - TIE) <= med <= max(old_ms) * (1.0 + TIE)
    out["metropolis_line_unchanged"] = {
        "kernel": new[0]["kernel"], "parent_kernel": old[0]["kernel"], "parent_version": old[0]["version"], "version": new[0]["version"],
        "kernel_ms_per_sweep_runs": new_ms, "parent_kernel_ms_per_sweep_runs": old_ms, "median": med,
        "parent_min": min(old_ms), "parent_max": max(old_ms), "margin": TIE, "median_within_parent_min_max_and_margin": inside,
        "final_spins_and_energies_equal": True}
    print(json.dumps(out, indent=1))
    if not a.no_write:
        with open(OUT, "w") as f:
            json.dump(out, f, indent=1)
    assert inside, ("the Metropolis line's median left the parent's own min .. max by more than 1 %", new_ms, old_ms)


if __name__ == "__main__":
    main()
