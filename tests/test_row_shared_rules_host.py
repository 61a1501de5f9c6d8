"""Row-shared windows under the Glauber and heat-bath rules, what holds without a GPU: the version, that no option was
added, that sga_route_query did not grow (a query carries no rule: rs_grid is still its last word) and that
sga_explain_route keeps giving the Metropolis answer for an integer and a grid query under option "row_shared" = 1."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

# sga_option_name(0 ...) as it was before the rules were opened to the windows
OPTIONS = ["look_ahead", "clf_waves", "sparse_route", "batched_energy", "force_general", "csr_updates_per_step",
           "tsp_updates_per_step", "force_csr_bits", "csr_bits", "csr_slots", "half_integer_table", "force_csr_acc",
           "force_dense_canonical", "zero_slot_every", "replica_routing", "fields_scratch_mb", "clf_batched", "clf_tail_waves",
           "clf_fixed_point", "row_shared", "row_shared_grid", "row_shared_fields", "row_shared_tile_sites", "row_shared_window",
           "batch_fixed_point", "ragged_field_cache"]


@pytest.fixture(scope="module")
def N():
    import spin_glass_anneal_rl_amd as sg
    return sg._native


def test_version(N):
    assert N.lib().sga_version() >= 2000


def test_no_option_was_added(N):
    assert N.option_names() == OPTIONS


def test_the_route_query_did_not_grow(N, tmp_path):
    Q = N.RouteQuery
    assert Q.rs_grid.size == 4 and Q.rs_grid.offset == Q.rest_max_row.offset + 4 == ctypes.sizeof(Q) - 4
    assert [name for name, *_ in Q._fields_][-1] == "rs_grid"
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    src = tmp_path / "size.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "sga.h"\nint main() { std::printf("%zu %zu\\n", '
                   'sizeof(sga_route_query), offsetof(sga_route_query, rs_grid)); }\n')
    exe = str(tmp_path / "size")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    size, offset = map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    assert (size, offset) == (ctypes.sizeof(Q), Q.rs_grid.offset) and offset == size - 4


def test_explain_route_keeps_the_metropolis_answer(N):
    with open(os.path.join(ROOT, "tests", "golden", "route_table.json")) as f:
        c = next(c for c in json.load(f)["cases"] if c["name"].startswith("BASELINE c2a"))
    integer = N.explain_route(N.route_query(**{**c["query"], "options": {"row_shared": 1}}))
    assert integer == ("dense storage=f32 acc=f32 waves=8 chunks_per_wave=5 ld=10240 look_ahead=2 kernel=sweep_dense_kernel "
                       "sweep=row-shared(W=1024) cached=off")
    grid = N.explain_route(N.route_query(**{**c["query"], "acc": 1, "table_m": 0, "rs_grid": 3,
                                            "options": {"row_shared": 1, "row_shared_grid": 1}}))
    assert grid == ("dense storage=f32 acc=f64-exact waves=8 chunks_per_wave=5 ld=10240 look_ahead=1 kernel=sweep_dense_kernel "
                    "sweep=row-shared(W=1024 grid=2^-2) cached=off")
    assert "rule=" not in integer + grid
