"""The engine-reuse walks without a GPU: what they cover, whether the comparison can fail, and whether free_problem()
in csrc/sga_engine_impl.h resets every problem-scoped member of the engine record."""
import os
import re

import numpy as np
import pytest

import engine_reuse as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPL = os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc", "sga_engine_impl.h")


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


# ----------------------------------------------------------------------------- the engine record against free_problem()
# Members of the "// problem" section that are NOT the problem's, each with the reason it may survive a setter.
# The caller's own settings persist by contract (include/sga.h):
PERSIST = {
    "csr_storage": "sga_set_csr_storage: the caller's choice for every later CSR problem",
    "field_cache": "sga_set_field_cache: the caller's choice for every later problem",
    "rule": "sga_set_update_rule: the caller's choice for every later problem",
    "tune_spl": "sga_set_tuning's sweeps per launch (sga_autotune puts the caller's value back itself)",
}
# ... these live as long as the engine:
ENGINE_LIFETIME = {
    "aux_stream": "the second stream of a mixed launch, created once, destroyed in sga_destroy",
    "fork_ev": "event of the mixed launch, created once, destroyed in sga_destroy",
    "join_ev": "event of the mixed launch, created once, destroyed in sga_destroy",
    "last_kernel": "what this engine's last sweep launched: a record of the past, not a trait of the problem",
}
# ... and these belong to the replicas: free_replicas(), which every setter calls first, must assign them
REPLICA_SCOPED = ("fields", "fields_valid", "ybuf", "ybuf_bytes", "routing", "d_rep_lists")


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


def _members(section):
    """Names of the data members declared in a piece of the struct (comments, member functions and initialisers dropped)."""
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
            names.append(m.group(1))
    return names


def _assigned(body, name, text):
    # (win: the window forms' state resets itself by lifetime, next_problem / next_replicas -- member by member in
    #  tests/test_window_forms_host.py::test_what_each_reset_drops)
    pat = (rf"\b{name}\b(\[[^\]]*\])?\s*=(?!=)|dev_free\({name}\)|\b{name}\.(clear|reset|assign|next_\w+)\(")
    if re.search(pat, body):
        return True
    # members reset through a helper the body calls (free_row_shared())
    return any(re.search(pat, _body(text, f"void {fn}()")) for fn in re.findall(r"\b(free_\w+)\(\)", body)
               if f"void {fn}()" in text and fn not in ("free_problem", "free_replicas"))


def _record():
    text = open(IMPL).read()
    struct = _body(text, "struct sga_engine {")
    begin, end = struct.index("    // problem\n"), struct.index("    // replicas\n")
    return text, _members(struct[begin:end])


def test_the_parser_reads_the_section():
    _, members = _record()
    for name in ("n", "n_models", "model_row0", "d_models", "J_bits", "table_scale", "tsp_args", "g_exp", "tune_table", "win",
                 "scan_words", "csr_x_exact", "last_kernel", "clf_ragged_why", "cpw_t2", "nd4t", "rowptr64"):
        assert name in members, name
    assert "implicit" not in members and "free_row_shared" not in members and len(members) == len(set(members)) > 90
    assert _members("int a = 0, *b = nullptr;  // x\n std::vector<int> c, d; void f() { a = 1; }\n char e[8] = {0}; T g{};") == \
        ["a", "b", "c", "d", "e", "g"]


def test_free_problem_resets_every_problem_scoped_member():
    """Every member declared in the struct's "// problem" section is assigned in free_problem() -- or is on one of the
    short lists above, with its reason.  A member added later without either fails here."""
    text, members = _record()
    body = _body(text, "void free_problem()")
    replicas = _body(text, "void free_replicas()")
    listed = set(PERSIST) | set(ENGINE_LIFETIME) | set(REPLICA_SCOPED)
    assert listed <= set(members), ("listed, but no longer a member of the section", listed - set(members))
    assert all(len(r) > 20 for r in list(PERSIST.values()) + list(ENGINE_LIFETIME.values()))
    missing = [m for m in members if m not in listed and not _assigned(body, m, text)]
    assert not missing, ("problem-scoped members that free_problem() does not reset", missing)
    missing = [m for m in REPLICA_SCOPED if not _assigned(replicas, m, text)]
    assert not missing, ("replica-scoped members that free_replicas() does not reset", missing)
    # the autotuner's pick ends with its problem: free_problem() goes back to the caller's own values
    assert re.search(r"tune_waves\s*=\s*caller_tune_waves", body) and re.search(r"opt\[OPT_CSR_UPDATES_PER_STEP\]\s*=\s*caller_csr_ups", body)


def test_the_check_would_notice_a_member_left_out():
    text, members = _record()
    body = _body(text, "void free_problem()")
    for gone in ("table_scale = 1;", "from_dense = false;", "dev_free(g_rent);", "model_n.clear();"):
        assert gone in body, gone
        name = re.search(r"[a-z_]\w*(?=\)| =|\.)", gone.replace("dev_free(", "")).group(0)
        assert _assigned(body, name, text) and not _assigned(body.replace(gone, ""), name, text), name
