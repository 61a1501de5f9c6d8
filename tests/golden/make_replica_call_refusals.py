#!/usr/bin/env python3
"""Records tests/golden/replica_call_refusals.json: the return code and sga_last_error() of every case of the grid in
tests/replica_refusal_cases.py, as the library of one commit answers it on the GPU.

Build the library of the commit to record (the parent of a refactoring) somewhere, and run, from the repository root,

    SGA_LIBRARY_PATH=/path/to/that/libsga.so python3 tests/golden/make_replica_call_refusals.py --commit <its 40-digit id>

tests/test_replica_call_refusals_gpu.py replays the table on the tree's own library."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import replica_refusal_cases as cases  # noqa: E402
import spin_glass_anneal_rl_amd as sg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose library answers")
    ap.add_argument("--out", default=os.path.join(HERE, "replica_call_refusals.json"))
    a = ap.parse_args()
    assert len(a.commit) == 40, "the full commit id"
    run = cases.Runner(sg)
    rows = []
    for call, engine, args in cases.grid():
        code, error = run.run(call, engine, args)
        rows.append({"call": call, "engine": engine, "args": args, "code": code, "error": error})
    run.close()
    table = {"note": f"answers of commit {a.commit[:7]} ({os.path.basename(sg._native.library_path())} built from it), recorded on an MI355X",
             "commit": a.commit, "rows": rows}
    with open(a.out, "w") as f:
        json.dump(table, f, indent=0)
        f.write("\n")
    refused = sum(r["code"] != 0 for r in rows)
    print(f"{len(rows)} cases, {refused} refused, {len({r['error'] for r in rows})} distinct texts -> {a.out}")
    launched = [r for r in rows if r["code"] == 0 and not cases.returns_early(r["args"])]  # nothing of the grid may reach a launch
    for r in launched:
        print("SERVED, not refused:", r["call"], r["engine"], r["args"])
    sys.exit(1 if launched else 0)


if __name__ == "__main__":
    main()
