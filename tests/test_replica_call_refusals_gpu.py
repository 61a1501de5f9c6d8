"""Every refusal of the seventeen replica and quantum calls (csrc/sga_replicas.cpp, csrc/sga_quantum.cpp), string for string
against the commit before their host side was written once: tests/golden/replica_call_refusals.json holds that commit's
return code and sga_last_error() for every case of the grid in tests/replica_refusal_cases.py (recorded by
tests/golden/make_replica_call_refusals.py on an MI355X), and the tree's library is held against it case by case -- the
code, the text and, through the two-fault cases, the order of the checks.  Refused calls launch nothing."""
import json
import os
import re

import pytest

import replica_refusal_cases as cases
from conftest import GOLDEN


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN, "replica_call_refusals.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def answers():
    import spin_glass_anneal_rl_amd as sg
    run = cases.Runner(sg)
    yield run.run
    run.close()


def test_the_table_is_the_grid(table):
    assert re.fullmatch(r"[0-9a-f]{40}", table["commit"]) and table["commit"][:7] in table["note"]
    assert [[r["call"], r["engine"], r["args"]] for r in table["rows"]] == json.loads(json.dumps(cases.grid()))
    assert {r["call"] for r in table["rows"]} == set(cases.CALLS) and len(cases.CALLS) == 17
    assert len(table["rows"]) >= 350
    # only a call with nothing to do is served, every other case is a refusal with a text; each call has refusals
    for r in table["rows"]:
        assert (r["code"] == 0 and r["error"] == "" and cases.returns_early(r["args"])) or (r["code"] in (-1, -4) and r["error"]), r
    for call in cases.CALLS:
        assert sum(r["call"] == call and r["code"] != 0 for r in table["rows"]) >= 7
    # the three ladder calls: every rung of the ladder rule, and the empty range that is served
    for call, noun in (("sga_cluster_move_ladders", "cluster moves"), ("sga_accumulate_ladder_overlaps", "overlaps"),
                       ("sga_accumulate_ladder_class_overlaps", "overlaps")):
        texts = {r["error"] for r in table["rows"] if r["call"] == call}
        assert {"no ladder (call sga_set_ladder)", noun + " between ladders need an even number of ladders",
                noun + " between ladders need every replica on this rank (R_local == R_global)", "slot range outside [0, slots)", ""} <= texts
    assert len({r["error"] for r in table["rows"]}) >= 100


@pytest.mark.gpu
def test_every_answer_of_the_parent_commit_is_reproduced(table, answers):
    wrong = []
    for r in table["rows"]:
        got = answers(r["call"], r["engine"], r["args"])
        if got != (r["code"], r["error"]):
            wrong.append((r["call"], r["engine"], r["args"], got, (r["code"], r["error"])))
    assert not wrong, wrong[:5]
