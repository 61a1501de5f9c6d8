"""Row-shared windows on a binary grid (option "row_shared_grid"), what holds without a GPU: the version and the option,
the ABI of the query field, the route's answers for hand-filled queries, the set-time verdict
(tests/c_abi/rs_grid_classify.cpp over sga_classify.cpp, scans built by tests/scan_reference.py) and the config flags."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import scan_reference as ref
from conftest import ROOT

GRID = "row-shared windows (grid): "


@pytest.fixture(scope="module")
def N():
    import spin_glass_anneal_rl_amd as sg
    return sg._native


def _cases():
    with open(os.path.join(ROOT, "tests", "golden", "route_table.json")) as f:
        return json.load(f)["cases"]


def _c2a():
    return next(c for c in _cases() if c["name"].startswith("BASELINE c2a"))


def test_version_and_option(N):
    assert N.lib().sga_version() >= 1800
    names = N.option_names()
    assert names.index("row_shared_grid") == names.index("row_shared") + 1
    assert names[-3:] == ["row_shared_window", "batch_fixed_point", "ragged_field_cache"]
    assert N.route_query().opt[names.index("row_shared_grid")] == 0  # the default
    text = open(os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc", "sga_route.h")).read()
    assert '{"row_shared_grid", "SGA_ROW_SHARED_GRID", 0, 0, 0, 0, 1, 0},' in text  # default 0, range [0, 1], [sweep]
    header = open(os.path.join(ROOT, "include", "sga.h")).read()
    assert re.search(r'"row_shared_grid"\s+0 \(default\) \| 1', header) and "[sweep; SGA_ROW_SHARED_GRID]" in header


def test_the_query_field_took_the_place_of_the_reserved_word(N, tmp_path):
    """Same size, same offset (the last word of the struct), zeroed by the init call -- and the ctypes struct still has
    the size a C compiler gives sga_route_query."""
    Q = N.RouteQuery
    assert Q.rs_grid.size == 4 and Q.rs_grid.offset == Q.rest_max_row.offset + 4 == ctypes.sizeof(Q) - 4
    assert N.route_query().rs_grid == 0 and N.route_query(rs_grid=3).rs_grid == 3
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    src = tmp_path / "size.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "sga.h"\nint main() { std::printf("%zu %zu\\n", '
                   'sizeof(sga_route_query), offsetof(sga_route_query, rs_grid)); }\n')
    exe = str(tmp_path / "size")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    size, offset = map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    assert (size, offset) == (ctypes.sizeof(Q), Q.rs_grid.offset)


def test_explain_route_names_the_grid_form_only_where_it_runs(N):
    c = _c2a()
    grid = {**c["query"], "acc": 1, "table_m": 0, "rs_grid": 3}
    on = {"row_shared": 1, "row_shared_grid": 1}
    named = N.explain_route(N.route_query(**{**grid, "options": on}))
    assert " sweep=row-shared(W=1024 grid=2^-2) cached=off" in named, named
    assert "acc=f64-exact" in named and "look_ahead=1" in named
    assert N.explain_route(N.route_query(**{**grid, "rs_grid": 1, "options": on})).count("grid=2^-0)") == 1  # k = 0
    for change in ({"options": {"row_shared": 1, "row_shared_grid": 0}}, {"options": {"row_shared": 1}},
                   {"options": {"row_shared": 2, "row_shared_grid": 1}}, {"options": {"row_shared": 0, "row_shared_grid": 1}},
                   {"rs_grid": 0}, {"n_models": 2}, {"clf_ok": 0}, {"options": {**on, "look_ahead": 0}},
                   {"options": {**on, "force_general": 1}}, {"field_cache": 1}, {"field_cache": 2}):
        q = {**grid, "options": on, **change}
        assert "row-shared" not in N.explain_route(N.route_query(**q)), change
    shared = N.explain_route(N.route_query(**{**grid, "options": on, "n_models": 4, "shared_j": 1}))
    assert " shared-J models=4 sweep=row-shared(W=1024 grid=2^-2)" in shared, shared
    # the integer clause is as it was, whatever the new option and field say
    forced = N.explain_route(N.route_query(**{**c["query"], "options": {"row_shared": 1}}))
    assert N.explain_route(N.route_query(**{**c["query"], "rs_grid": 3, "options": on})) == forced
    assert " sweep=row-shared(W=1024) " in forced


def test_every_recorded_answer_stays_as_it_is(N):
    cases = _cases()
    assert len(cases) >= 25
    for c in cases:
        assert N.explain_route(N.route_query(**c["query"])) == c["explain"], c["name"]
        assert N.explain_route(N.route_query(**{**c["query"], "rs_grid": 3})) == c["explain"], c["name"]  # (option at 0)


# ----------------------------------------------------------------------------- the set-time verdict
def _sym(U):
    U = np.triu(np.asarray(U, np.float32), 1)
    return U + U.T


def _verdict_cases():
    rng = np.random.RandomState(5)
    n = 12
    pm = _sym(rng.randint(0, 2, (n, n)) * 2 - 1)
    ints = rng.randint(-2, 3, n).astype(np.float32)
    small = _sym(rng.randint(-3, 4, (n, n)))
    small[0, 1] = small[1, 0] = 3.0
    # 2^k row_abs_max against 2^24 at k = 2: a row of four couplings of 1/4 beside one field value.  fx_bound allows for
    # the fp32 rounding of the word (a factor 1 + 2^-20, 16 units at 2^24): 2^24 - 16 is the last scaled value it
    # admits, 2^24 - 15 the first it refuses (in quarters: 2^22 - 4 and 2^22 - 3.75, both exact in fp32)
    edge = _sym(np.full((5, 5), 0.25))

    def edge_h(row_abs_max):
        h = np.zeros(5, np.float32)
        h[0] = np.float32(row_abs_max - 1.0)
        assert float(h[0]) + 1.0 == row_abs_max
        return h

    asym = pm * 0.25
    asym[0, 1] = -asym[1, 0]
    F32, I8 = 1, 2  # SGA_J_F32, SGA_J_I8
    return [
        ("quarter J, |4 J| <= 1", pm * 0.25, ints * 0.25, F32, "k=2 planes=1 why=-"),
        ("quarter J, |4 J| <= 7", _sym(rng.randint(-7, 8, (n, n))) * 0.25, ints * 0.25, F32, "k=2 planes=3 why=-"),
        ("eighths, |8 J| <= 100", _sym(np.where(np.eye(n, k=1), 100, rng.randint(-100, 101, (n, n)))) * 0.125, ints, F32,
         "k=3 planes=8 why=-"),
        ("integer J, integer h", small, ints, F32, "k=0 planes=0 why=" + GRID + "an integer problem, the integer form of the windows serves it"),
        ("integer J, h = 0.3", small, np.full(n, 0.3, np.float32), F32, "k=0 planes=3 why=-"),
        ("integer J as int8, h = 0.3", small, np.full(n, 0.3, np.float32), I8, "k=0 planes=3 why=-"),
        ("J = +-2^-20", pm * 2.0 ** -20, ints * 2.0 ** -20, F32, "k=20 planes=1 why=-"),
        ("scaled max 255", np.where(pm != 0, pm * 255 * 0.25, 0), ints, F32, "k=2 planes=8 why=-"),
        ("scaled max 256", _sym(np.where(np.eye(n, k=1), 256, 1)) * 0.25, ints, F32,
         "k=0 planes=0 why=" + GRID + "2^k max |J_ij| exceeds 255 (bit-planes of |2^k J|)"),
        ("Gaussian J", _sym(rng.randn(n, n)), ints, F32, None),
        ("asymmetric J", asym, ints, F32, "k=0 planes=0 why=" + GRID + "J must be symmetric with a zero diagonal"),
        ("J all zero", np.zeros((n, n), np.float32), np.full(n, 0.3, np.float32), F32, "k=0 planes=0 why=" + GRID + "J is all zero"),
        ("J = +-2^-31", pm * 2.0 ** -31, ints, F32, "k=0 planes=0 why=" + GRID + "the couplings need a grid finer than 2^-30"),
        ("bound at 2^24", edge, edge_h(2.0 ** 22), F32,
         "k=0 planes=0 why=" + GRID + "2^k max_i (sum_j |J_ij| + |h_i|) is not below 2^24"),
        ("bound one step below", edge, edge_h(2.0 ** 22 - 4.0), F32, "k=2 planes=1 why=-"),
        ("bound first refused", edge, edge_h(2.0 ** 22 - 3.75), F32,
         "k=0 planes=0 why=" + GRID + "2^k max_i (sum_j |J_ij| + |h_i|) is not below 2^24"),
        ("h = 3e5 at k = 6", pm * 2.0 ** -6, np.full(n, 3.0e5, np.float32), F32,
         "k=0 planes=0 why=" + GRID + "2^k max_i (sum_j |J_ij| + |h_i|) is not below 2^24"),
    ]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_grid_verdicts(tmp_path):
    csrc = os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc")
    exe = str(tmp_path / "rs_grid_classify")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "c_abi", "rs_grid_classify.cpp"), "-o", exe, "-L", csrc, "-lsga",
                    "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    cases = _verdict_cases()
    args = []
    for _, J, h, storage, _ in cases:
        args += [J.shape[0], storage] + ref.dense_words(J, h)
    out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(cases)
    for line, (name, J, h, _, want) in zip(out, cases):
        head, got = line.split(": ", 1)
        assert f"j_max={float(np.abs(J).max()):.9g}" in head, (name, line)  # word [7] as the float the scan wrote
        if want is None:  # Gaussian J: some condition refuses it (which one first depends on the draw)
            assert got.startswith("k=0 planes=0 why=" + GRID), (name, line)
        else:
            assert got == want, (name, line)


def test_config_flags_default_to_false():
    import spin_glass_anneal_rl_amd as sg
    assert sg.GPUAnnealerConfig().row_shared_grid is False
    assert sg.ParallelTemperingConfig().row_shared_grid is False
    assert sg.GPUAnnealerConfig(row_shared_grid=True).row_shared_grid is True
    assert sg.ParallelTemperingConfig(row_shared_grid=True).row_shared_grid is True
