"""The engine-reuse walks without a GPU: what they cover, whether the comparison can fail, and whether the two resets
of the engine record in csrc/sga_engine_impl.h (free_problem, free_replicas) drop every member of the sub-record they
stand for, release every buffer it owns once, and leave the rest of the engine alone (tests/c_abi/engine_record.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import engine_reuse as er
from test_window_forms_host import HIPCC, HOST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPL = os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc", "sga_engine_impl.h")
PROGRAM = os.path.join(ROOT, "tests", "c_abi", "engine_record.cpp")


# ----------------------------------------------------------------------------- coverage
def test_the_circuit_covers_every_ordered_pair_of_kinds_once():
    kinds = er.euler_kinds()
    arcs = list(zip(kinds, kinds[1:]))
    assert len(arcs) == 42 == len(set(arcs)) and all(a != b for a, b in arcs) and kinds[0] == kinds[-1]
    assert set(arcs) == {(a, b) for a in er.KINDS for b in er.KINDS if a != b}


def test_the_walks_cover_all_42_pairs_and_chain_up():
    assert len(er.EULER) == 3 and all(14 <= len(w) <= 16 for w in er.EULER)
    assert all(a[-1] == b[0] for a, b in zip(er.EULER, er.EULER[1:]))
    assert er.kind_pairs(er.EULER) == {(a, b) for a in er.KINDS for b in er.KINDS if a != b}
    assert er.EULER == er.euler_walks()  # a fixed rule, no RNG
    for w in er.EULER:  # the one edge a walk cannot take (sga_set_field_cache(ON) while a ragged batch is held)
        assert not any(a == "G1" and b in er.NEEDS_CACHE_ON for a, b in zip(w, w[1:]))


def test_every_station_is_a_predecessor_and_a_successor():
    walks = er.EULER + er.FIXED
    assert all(sid in er.BY_ID for w in walks for sid in w)
    pred = {a for w in walks for a in w[:-1]}
    succ = {b for w in walks for b in w[1:]}
    assert pred == set(er.BY_ID) == succ, (set(er.BY_ID) - pred, set(er.BY_ID) - succ)
    assert {s.kind for s in er.STATIONS} == set(er.KINDS)


def test_sizes_go_down_as_well_as_up_and_R_cycles():
    assert er.R_CYCLE == (3, 33, 8)
    kinds = [[er.BY_ID[s].kind for s in w] for w in er.EULER]
    # (a CSR or dense station is followed by the small implicit ones and the other way round, in every walk)
    small = {"tsp", "groups", "groups_rest"}
    for k in kinds:
        steps = list(zip(k, k[1:]))
        assert any(a not in small and b in small for a, b in steps) and any(a in small and b not in small for a, b in steps)


# ----------------------------------------------------------------------------- the comparison helper
def _state():
    return {"describe": "dense n=4 models=1", "route_query.n": 4, "route_query.table_scale": 1, "option.look_ahead": 1,
            "scan_summary[0]": (0, [1, 1, 0, 1]), "spins": np.ones((2, 4), np.int8), "spins_of": [np.ones(4, np.int8)] * 2,
            "energies": np.asarray([-1.5, 2.0]), "counters": (3, 1), "swapped": 0, "slot_map": np.arange(2, dtype=np.int32)}


def test_assert_same_engine_passes_on_equal_states():
    er.assert_same_engine(_state(), _state(), "equal")


@pytest.mark.parametrize("key", ["spins", "spins_of", "energies", "route_query.table_scale", "option.look_ahead", "describe",
                                 "scan_summary[0]", "counters", "swapped", "slot_map"])
def test_assert_same_engine_names_the_one_differing_key(key):
    a, b = _state(), _state()
    if key == "spins":
        b[key] = b[key].copy()
        b[key][1, 2] = -1                                        # one spin
    elif key == "spins_of":
        b[key] = [b[key][0], -b[key][1]]
    elif key == "energies":
        b[key] = np.nextafter(b[key], np.inf) * [1, 0] + b[key] * [0, 1]   # one bit of one energy
        assert np.sum(b[key] != a[key]) == 1 and np.allclose(a[key], b[key], rtol=1e-15, atol=0)
    elif key == "route_query.table_scale":
        b[key] = 2                                               # one route_query field
    elif key == "option.look_ahead":
        b[key] = 0                                               # one option
    elif key == "describe":
        b[key] += " "
    elif key == "scan_summary[0]":
        b[key] = (0, [1, 1, 0, 0])
    elif key == "counters":
        b[key] = (3, 0)
    elif key == "swapped":
        b[key] = None
    else:
        b[key] = b[key].astype(np.int64)                         # the same values in another type
    with pytest.raises(AssertionError) as err:
        er.assert_same_engine(a, b, "walk X: visit 3 (D1 -> T1)")
    assert f"first differing key {key!r}" in str(err.value) and "walk X: visit 3 (D1 -> T1)" in str(err.value)
    with pytest.raises(AssertionError):
        er.assert_same_engine(b, a, "the other way round")


def test_assert_same_engine_tells_a_negative_zero_and_a_missing_key():
    a, b = _state(), _state()
    a["energies"], b["energies"] = np.asarray([0.0, 2.0]), np.asarray([-0.0, 2.0])
    with pytest.raises(AssertionError, match="energies"):
        er.assert_same_engine(a, b, "zero")
    b = _state()
    del b["swapped"]
    with pytest.raises(AssertionError, match="swapped"):
        er.assert_same_engine(_state(), b, "keys")


# ----------------------------------------------------------------------------- the engine record against its two resets
# sga_engine derives from ProblemState and ReplicaState; each resets by releasing the buffers it owns and assigning a fresh
# record.  tests/c_abi/engine_record.cpp runs free_replicas() / free_problem() over a filled engine (sentinels, no device
# memory) and prints what came back to its default, what kept its value and what was released.  The declarations are read
# here only for their member names: a member added later that the program does not cover fails below.
REPLICA = ("spins best_spins energy best_energy rep_temp n_acc slot_temps slot_to_rep ex_attempts ex_accepts wolff_u wolff_cursor "
           "wolff_cap fields fields_valid ybuf ybuf_bytes routing d_rep_lists R Rg n_ladders").split()
# what sga_init_replicas writes and only the next problem resets
LATCHED = "waves cpw ld waves_t2 cpw_t2 big big_form table_m tsp_waves tsp_passes csr_storage_latched".split()
# what no reset may touch: the caller's choices, what lives as long as the engine, the window state's own two, the
# random stream's coordinates and the counters
SURVIVE = ("opt opt_stale opt_stale_key caller_tune_waves caller_csr_ups csr_storage field_cache rule tune_waves tune_spl "
           "own_stream stream aux_stream fork_ev join_ev last_kernel d_count d_flags scratch point_sites point_out csr_energy "
           "timing events launches total_ms win.seq_w win.suspend replica0 seed sstride attempted sweeps_done rounds").split()
# free_problem() puts the caller's own values back over the autotuner's pick: these two hold neither their value nor a default
CALLERS = ["opt", "tune_waves"]


def _braces(text, at):
    """The index just past the brace block that opens at text[at] == '{'."""
    depth = 0
    for i in range(at, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return i + 1
    raise AssertionError("unbalanced braces")


def _body(text, signature):
    at = text.index(signature)
    open_ = text.index("{", at)
    return text[open_:_braces(text, open_)]


def _members(section, owned_pointers=False):
    """Names of the data members declared in a piece of a struct (comments, member functions and initialisers dropped).
    owned_pointers: only those declared with a '*' to something not const (const char *: a string literal, not a buffer)."""
    s = re.sub(r"//[^\n]*", "", section)
    s = re.sub(r"\{\s*0?\s*\}", "", s)  # value initialisers: tsp_args{}, last_kernel[512] = {0}
    while "{" in s:  # what is left in braces is a member function's body: drop the function
        open_ = s.index("{")
        start = max(s.rfind(";", 0, open_), s.rfind("}", 0, open_)) + 1
        s = s[:start] + s[_braces(s, open_):]
    names = []
    for decl in s.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in re.sub(r"<[^<>]*>", "", decl).split(","):
            part = part.split("=")[0].strip()
            m = re.search(r"([A-Za-z_]\w*)\s*(\[[^\]]*\])?$", part)
            assert m, (decl, part)
            if not owned_pointers or ("*" in part and not decl.startswith("const ")):
                names.append(m.group(1))
    return names


def _declared(struct, **kw):
    """Member names of `struct ProblemState {` | `struct ReplicaState {` | `struct sga_engine :` as declared."""
    return _members(_body(open(IMPL).read(), f"struct {struct}")[1:-1], **kw)


def _run(exe, *args):
    """The program's report: key -> the names behind it"""
    run = subprocess.run([exe, *args], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    return {key: names.split() for key, names in (ln.split(":", 1) for ln in run.stdout.splitlines())}, run.stdout


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("engine_record") / "engine_record")
    subprocess.run([HIPCC] + HOST + [PROGRAM, "-o", exe], check=True, capture_output=True)
    return exe


def test_the_parser_reads_the_section():
    problem, replica, engine = _declared("ProblemState {"), _declared("ReplicaState {"), _declared("sga_engine :")
    for name in ("n", "n_models", "model_row0", "d_models", "J_bits", "table_scale", "tsp_args", "g_exp", "tune_table",
                 "scan_words", "csr_x_exact", "clf_ragged_why", "cpw_t2", "nd4t", "rowptr64", "group_args", "epart_bytes"):
        assert name in problem, name
    for name in ("win", "last_kernel", "opt", "scratch", "events", "join_ev", "rounds", "csr_energy"):
        assert name in engine, name
    everything = problem + replica + engine
    assert not {"implicit", "reset", "free_row_shared", "free_problem", "free_replicas", "release"} & set(everything)
    assert len(everything) == len(set(everything)) and len(problem) > 80 and len(replica) == 22 and len(engine) > 30
    toy = "int a = 0, *b = nullptr;  // x\n std::vector<int> c, d; void f() { a = 1; }\n char e[8] = {0}; T g{}; const char *w = nullptr; void *p;"
    assert _members(toy) == ["a", "b", "c", "d", "e", "g", "w", "p"] and _members(toy, owned_pointers=True) == ["b", "p"]
    assert "clf_why" not in _declared("ProblemState {", owned_pointers=True) and "d_models" in _declared("ProblemState {", owned_pointers=True)


def test_the_program_covers_exactly_the_declared_members(record):
    out, _ = _run(record)
    assert sorted(out["members.problem"]) == sorted(_declared("ProblemState {"))
    assert sorted(out["members.replica"]) == sorted(_declared("ReplicaState {")) == sorted(REPLICA)
    # (win resets itself by lifetime -- tests/test_window_forms_host.py::test_what_each_reset_drops; here its two members that
    #  no reset touches stand for it)
    own = sorted(set(_declared("sga_engine :")) - {"win"} | {"win.seq_w", "win.suspend"})
    assert sorted(out["members.engine"]) == own and set(SURVIVE) <= set(own)
    assert set(LATCHED) <= set(out["members.problem"])
    assert out["members.unfilled"] == []  # every member was given a value that is not its default


def _owned(struct):
    return [m for m in _declared(struct, owned_pointers=True) if m != "d_models"]  # (a view into h's allocation)


def test_free_problem_resets_every_problem_scoped_member(record):
    """Every ProblemState member is back at its declared default after free_problem(), every buffer the record owns went
    to the release function once, the replicas and the rest of the engine kept their values -- but for tune_waves and
    option "csr_updates_per_step", which are the caller's own again."""
    out, _ = _run(record)
    f = "free_problem"
    assert out[f + ".problem.reset"] == out["members.problem"] and not out[f + ".problem.kept"] and not out[f + ".problem.neither"]
    assert out[f + ".replica.kept"] == out["members.replica"] and not out[f + ".replica.reset"] and not out[f + ".replica.neither"]
    assert sorted(out[f + ".released"]) == sorted(_owned("ProblemState {")) and len(out[f + ".released"]) == 23
    assert "d_models" not in out[f + ".released"] and "d_models" in out[f + ".problem.reset"]
    assert out[f + ".engine.kept"] == [m for m in out["members.engine"] if m not in CALLERS] and not out[f + ".engine.reset"]
    assert out[f + ".engine.neither"] == CALLERS
    assert out[f + ".caller"] == ["tune_waves=caller's", "csr_updates_per_step=caller's", "other_options=kept"]
    assert set(SURVIVE) - set(CALLERS) <= set(out[f + ".engine.kept"])


def test_free_replicas_resets_every_replica_scoped_member_and_nothing_else(record):
    out, _ = _run(record)
    f = "free_replicas"
    assert out[f + ".replica.reset"] == out["members.replica"] and not out[f + ".replica.kept"] and not out[f + ".replica.neither"]
    assert out[f + ".problem.kept"] == out["members.problem"] and not out[f + ".problem.reset"] and not out[f + ".problem.neither"]
    assert sorted(out[f + ".released"]) == sorted(_owned("ReplicaState {")) and len(out[f + ".released"]) == 15
    assert out[f + ".engine.kept"] == out["members.engine"] and not out[f + ".engine.reset"] and not out[f + ".engine.neither"]
    assert out[f + ".caller"] == ["tune_waves=kept", "csr_updates_per_step=kept", "other_options=kept"]


def test_both_resets_release_every_owned_buffer_exactly_once(record):
    """free_replicas() then free_problem(), as every setter and sga_destroy call them."""
    out, _ = _run(record)
    assert out["both.released"] == out["free_replicas.released"] + out["free_problem.released"]
    assert len(out["both.released"]) == len(set(out["both.released"])) == 38 and "?" not in out["both.released"]
    assert out["both.problem.reset"] == out["members.problem"] and out["both.replica.reset"] == out["members.replica"]
    assert out["both.engine.kept"] == out["free_problem.engine.kept"] and out["both.engine.neither"] == CALLERS
    assert not out["both.engine.reset"] and set(SURVIVE) - set(CALLERS) <= set(out["both.engine.kept"])


def test_the_check_would_notice_a_member_left_out(record):
    """Mode "selfcheck" puts one value member and one buffer back to their filled values after the resets: the report
    names exactly those two as kept."""
    out, _ = _run(record, "selfcheck")
    for f in ("free_problem", "both"):
        assert out[f + ".problem.kept"] == ["table_scale", "g_rent"] and not out[f + ".problem.neither"]
        assert out[f + ".problem.reset"] == [m for m in out["members.problem"] if m not in ("table_scale", "g_rent")]
    assert out["free_replicas.problem.kept"] == out["members.problem"]


def test_the_record_under_the_sanitizers(record, tmp_path):
    """The same stand-alone program built with the address and undefined-behaviour sanitizers: the same report, no finding."""
    exe = str(tmp_path / "engine_record_san")
    san = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run([HIPCC] + HOST + san + [PROGRAM, "-o", exe], check=True, capture_output=True)
    for mode in ((), ("selfcheck",)):
        assert _run(exe, *mode)[1] == _run(record, *mode)[1]


