"""Sequential windows (sga_set_sequential_windows, csrc/sweep_dense_seq.hip), what holds without a GPU: the version, the
two symbols in the library and in include/sga.h, that the setter is a setter of its own -- no option was added and
sga_route_query did not grow -- and that the public class validates its site order."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

# sga_option_name(0 ...) and sizeof(sga_route_query) as they were before the form
OPTIONS = ["look_ahead", "clf_waves", "sparse_route", "batched_energy", "force_general", "csr_updates_per_step",
           "tsp_updates_per_step", "force_csr_bits", "csr_bits", "csr_slots", "half_integer_table", "force_csr_acc",
           "force_dense_canonical", "zero_slot_every", "replica_routing", "fields_scratch_mb", "clf_batched", "clf_tail_waves",
           "clf_fixed_point", "row_shared", "row_shared_grid", "row_shared_fields", "row_shared_tile_sites", "row_shared_window",
           "batch_fixed_point", "ragged_field_cache"]
# 15 int32, 3 int64, 6 int32, ldj, 32 option words, n_groups, group_max, rest_nnz, rest_max_row, rs_grid
ROUTE_QUERY_BYTES = 15 * 4 + 4 + 3 * 8 + 6 * 4 + 8 + 32 * 8 + 2 * 4 + 8 + 2 * 4


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def test_version(sg):
    assert sg._native.lib().sga_version() >= 2100


def test_both_symbols_are_exported_and_declared(sg):
    L = sg._native.lib()
    with open(os.path.join(ROOT, "include", "sga.h")) as f:
        header = f.read()
    for name in ("sga_set_sequential_windows", "sga_get_sequential_windows"):
        assert hasattr(L, name), name
        assert name in [s[0] for s in sg._native.SYMBOLS], name
    assert re.search(r"^int sga_set_sequential_windows\(sga_engine \*e, int W\);", header, re.M)
    assert re.search(r"^int sga_get_sequential_windows\(sga_engine \*e, int \*W\);", header, re.M)
    # a NULL engine is an error, not a crash (no device is touched)
    assert L.sga_set_sequential_windows(None, 256) == sg._native.ERR_INVALID
    assert L.sga_get_sequential_windows(None, None) == sg._native.ERR_INVALID


def test_no_option_and_no_query_field_was_added(sg):
    N = sg._native
    assert N.option_names() == OPTIONS
    assert ctypes.sizeof(N.RouteQuery) == ROUTE_QUERY_BYTES
    assert [name for name, *_ in N.RouteQuery._fields_][-1] == "rs_grid"


def test_the_public_class_validates_its_site_order(sg):
    with pytest.raises(sg.ConfigurationError):
        sg.ParallelTemperingConfig(site_order="diagonal")
    cfg = sg.ParallelTemperingConfig()
    assert (cfg.site_order, cfg.sequential_window) == ("random", 1024)
    assert sg.ParallelTemperingConfig(site_order="sequential", sequential_window=0).site_order == "sequential"
