"""Spin and link overlaps between pairs of replicas (sga_get_link_count / sga_get_pair_overlaps /
sga_accumulate_ladder_overlaps, csrc/pair_overlaps.hip), what holds without a GPU: the version, the three symbols in the
library, the header and the binding, that the calls added no option and no query field, the reference of
tests/overlap_reference.py against cases worked out by hand, the kernel's LDS bound, its lane groups and the host's checks
of a pair list and of the histogram arguments (tests/c_abi/pair_overlaps_plan.cpp), OverlapStatistics, and the
configuration checks of ParallelTemperingConfig (tests/test_pair_overlaps_gpu.py holds the engine against the reference)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import overlap_reference as ovr
from conftest import ROOT
from test_sequential_windows_host import OPTIONS, ROUTE_QUERY_BYTES

CSRC = os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc")
LDS_BUDGET = 160 * 1024 - 256      # what the cluster move allows itself
MAX_N = (LDS_BUDGET - 64) // 4 * 32  # the largest n whose bitmap of differing sites fits: 1 308 160


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("pair_overlaps_plan")), "pair_overlaps_plan")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-I", "/opt/rocm/include",
                    os.path.join(ROOT, "tests", "c_abi", "pair_overlaps_plan.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def plan(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.strip()


def ring(n, val=1.0):
    """CSR of a ring: site i joined to i - 1 and i + 1."""
    rowptr = np.arange(0, 2 * n + 1, 2, dtype=np.int32)
    col = np.stack([(np.arange(n) - 1) % n, (np.arange(n) + 1) % n], 1).reshape(-1).astype(np.int32)
    return rowptr, col, np.full(2 * n, val, np.float32)


def test_version(sg):
    assert sg._native.lib().sga_version() >= 2700


def test_the_three_symbols_are_exported_declared_and_bound(sg):
    L, N = sg._native.lib(), sg._native
    with open(os.path.join(ROOT, "include", "sga.h")) as f:
        header = f.read()
    names = [s[0] for s in N.SYMBOLS]
    for name in ("sga_get_link_count", "sga_get_pair_overlaps", "sga_accumulate_ladder_overlaps"):
        assert hasattr(L, name), name
        assert name in names, name
    assert re.search(r"^int sga_get_link_count\(sga_engine \*e, int64_t \*n_links", header, re.M)
    assert re.search(r"^int sga_get_pair_overlaps\(sga_engine \*e, int which[^;]*const int32_t \*pairs[^;]*int count,\s+"
                     r"int32_t \*dist[^;]*int64_t \*broken[^;]*\);", header, re.M)
    assert re.search(r"^int sga_accumulate_ladder_overlaps\(sga_engine \*e, int slot_lo, int slot_hi,\s+uint64_t \*hist_q, int bins_q, "
                     r"int q_shift,\s+uint64_t \*hist_l[^;]*int bins_l, int l_shift\);", header, re.M)
    assert "a duplicate (i, j) is\n *   TWO links" in header  # what packing does with duplicate input entries
    for name in ("link_count", "pair_overlaps", "accumulate_ladder_overlaps"):
        assert hasattr(sg.AnnealEngine, name), name
    assert hasattr(sg, "OverlapStatistics")


def test_no_option_and_no_query_field_was_added(sg):
    N = sg._native
    assert N.option_names() == OPTIONS
    assert ctypes.sizeof(N.RouteQuery) == ROUTE_QUERY_BYTES


# ---- the reference, against cases worked out by hand -------------------------------------------------------------------
def test_reference_arcs_of_a_ring():
    n = 12
    g = ring(n)
    s_a = np.ones(n, np.int8)
    s_b = s_a.copy()
    s_b[[2, 3, 4, 8, 9, 11, 0]] = -1  # arcs {2, 3, 4}, {8, 9} and, through the ring's closing bond, {11, 0}
    assert ovr.dist(s_a, s_b) == 7
    assert ovr.link_count(*g) == 24
    assert ovr.broken(*g, s_a, s_b) == 12  # each of the three arcs breaks two bonds, counted in both triangles
    assert ovr.dist(s_a, s_a) == 0 and ovr.broken(*g, s_a, s_a) == 0
    assert ovr.dist(s_a, -s_a) == n and ovr.broken(*g, s_a, -s_a) == 0  # every site differs: no bond is broken


def test_reference_a_stored_zero_is_no_link():
    # path 0 - 1 - 2 - 3 whose middle bond is stored as 0.0 / -0.0 / 0.5
    rowptr = np.asarray([0, 1, 3, 5, 6], np.int32)
    col = np.asarray([1, 0, 2, 1, 3, 2], np.int32)
    val = np.asarray([1, 1, 0, 0, -1, -1], np.float32)
    s_a = np.ones(4, np.int8)
    s_b = np.asarray([1, 1, -1, -1], np.int8)  # differs across the middle bond alone
    assert ovr.link_count(rowptr, col, val) == 4 and ovr.broken(rowptr, col, val, s_a, s_b) == 0
    val[2] = val[3] = -0.0
    assert ovr.link_count(rowptr, col, val) == 4 and ovr.broken(rowptr, col, val, s_a, s_b) == 0
    val[2] = val[3] = 0.5
    assert ovr.link_count(rowptr, col, val) == 6 and ovr.broken(rowptr, col, val, s_a, s_b) == 2


def test_reference_a_stored_diagonal_entry_is_no_link():
    # two sites, the bond both ways and a diagonal entry at site 0
    rowptr = np.asarray([0, 2, 3], np.int32)
    col = np.asarray([0, 1, 0], np.int32)
    val = np.asarray([3.0, 1.0, 1.0], np.float32)
    assert ovr.link_count(rowptr, col, val) == 2
    assert ovr.broken(rowptr, col, val, [1, 1], [-1, 1]) == 2 and ovr.dist([1, 1], [-1, 1]) == 1


def test_reference_accumulate():
    g = ring(4)
    S = np.asarray([[1, 1, 1, 1], [1, -1, 1, 1], [-1, -1, -1, -1], [1, 1, -1, -1]], np.int8)
    hq, hl = np.zeros((1, 2, 5), np.int64), np.zeros((1, 2, 9), np.int64)
    # two ladders of two slots; slot 0: replicas 1 and 2 (d = 3, b = 4), slot 1: replicas 0 and 3 (d = 2, b = 4)
    ovr.accumulate(hq, hl, [1, 0, 2, 3], 2, g, S)
    assert hq[0, 0].tolist() == [0, 0, 0, 1, 0] and hq[0, 1].tolist() == [0, 0, 1, 0, 0]
    assert hl[0, 0].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0] and hl[0, 1].tolist() == hl[0, 0].tolist()
    hq2 = np.zeros((1, 1, 2), np.int64)
    ovr.accumulate(hq2, None, [1, 0, 2, 3], 2, g, S, slot_lo=1, slot_hi=2, q_shift=1)
    assert hq2[0, 0].tolist() == [0, 1]  # d = 2 >> 1 = 1
    hq3 = np.zeros((1, 2, 2), np.int64)
    ovr.accumulate(hq3, None, [1, 0, 2, 3], 2, g, S)
    assert hq3[0].tolist() == [[0, 1], [0, 1]]  # clamped into the last bin


# ---- the kernel's host half ------------------------------------------------------------------------------------------
def test_lds_bytes_and_the_bound(plan_exe):
    ns = [1, 32, 33, MAX_N, MAX_N + 1]
    out = plan(plan_exe, "lds", *ns).split("\n")
    assert out[0].split() == [f"budget={LDS_BUDGET}", f"max_n={MAX_N}", "threads=256"]
    got = [tuple(int(v) for v in line.split()) for line in out[1:]]
    assert got == [(ovr.lds_bytes(n, True), ovr.lds_bytes(n, False)) for n in ns]
    assert [g[0] for g in got[:3]] == [4 + 64, 4 + 64, 8 + 64]  # one word of the bitmap up to n = 32, two from 33
    assert all(g[1] == 64 for g in got)                        # without links no bitmap, whatever n
    assert got[3][0] <= LDS_BUDGET < got[4][0] and MAX_N == 1_308_160
    assert got[3][0] - 64 == MAX_N // 8  # the bitmap is n / 8 bytes


def test_lanes_to_a_row(plan_exe):
    g = lambda entries, n: int(plan(plan_exe, "group", entries, n))  # noqa: E731
    assert g(0, 1) == 0 and g(5, 5) == 0          # no entries, one entry a row: a lane a row
    assert g(6 * 10648, 10648) == 3               # a degree-6 lattice: 8 lanes, not 16
    assert g(2 * 12, 12) == 1 and g(600, 301) == 1  # a ring; a star of 300 leaves (mean row 2)
    assert g(16 * 100, 100) == 4 and g(17 * 100, 100) == 5
    assert g(64 * 100, 100) == 6 and g(10 ** 12, 1000) == 6  # never more than a wave


def test_the_pair_list_check(plan_exe):
    assert plan(plan_exe, "pairs", 6, 0) == "ok"
    assert plan(plan_exe, "pairs", 6, 0, "null") == "ok"
    assert plan(plan_exe, "pairs", 6, 4, 0, 1, 1, 0, 0, 2, 3, 3) == "ok"  # a replica in many pairs, a == b: the call only reads
    assert "out of range" in plan(plan_exe, "pairs", 6, 1, 0, 6) and "out of range" in plan(plan_exe, "pairs", 6, 2, 0, 1, -1, 2)
    assert "negative" in plan(plan_exe, "pairs", 6, -1)
    assert "NULL" in plan(plan_exe, "pairs", 6, 1, "null")


def test_the_histogram_argument_check(plan_exe):
    assert plan(plan_exe, "hist", 1, 1, 0, 0, 0, 0) == "ok"      # no hist_l: its bins and shift are not looked at
    assert plan(plan_exe, "hist", 1, 13, 31, 1, 7, 31) == "ok"
    assert "NULL" in plan(plan_exe, "hist", 0, 4, 0, 1, 4, 0)
    assert "bin" in plan(plan_exe, "hist", 1, 0, 0, 0, 0, 0) and "bin" in plan(plan_exe, "hist", 1, 4, 0, 1, 0, 0)
    for q, l in ((32, 0), (-1, 0), (0, 32), (0, -1)):
        assert "shift" in plan(plan_exe, "hist", 1, 4, q, 1, 4, l)
    assert plan(plan_exe, "hist", 1, 4, 0, 0, 4, 32) == "ok"


# ---- OverlapStatistics -----------------------------------------------------------------------------------------------
def test_statistics_two_peaks(sg):
    n = 10
    h = np.zeros((2, 3, n + 1), np.uint64)
    h[:, :, 0] = h[:, :, n] = 7  # all weight at d = 0 (q = 1) and d = n (q = -1), in equal parts
    st = sg.OverlapStatistics(temperatures=np.asarray([2.0, 1.0, 0.5]), n=n, n_links=None, hist_q=h)
    assert np.array_equal(st.q_values(), 1.0 - 2.0 * np.arange(n + 1) / n)
    q2, q4 = st.moments()
    assert np.array_equal(q2, np.ones(3)) and np.array_equal(q4, np.ones(3)) and np.array_equal(st.binder(), np.ones(3))
    with pytest.raises(sg.ConfigurationError):
        st.link_values()


def test_statistics_binomial(sg):
    n = 40
    h = np.asarray([math.comb(n, d) for d in range(n + 1)], np.uint64).reshape(1, 1, n + 1)  # exact integers, all below 2^38
    st = sg.OverlapStatistics(temperatures=np.asarray([1.0]), n=n, n_links=None, hist_q=h)
    q2, q4 = st.moments()
    assert abs(q2[0] - 1.0 / n) < 1e-12               # Var d = n / 4, q = 1 - 2 d / n
    assert abs(q4[0] - (3.0 * n - 2.0) / n ** 3) < 1e-12  # the fourth central moment of the binomial
    assert abs(st.binder()[0] - 0.5 * (3.0 - (3.0 * n - 2.0) / n)) < 1e-9
    # two copy pairs are summed: the same weights twice give the same moments
    st2 = sg.OverlapStatistics(temperatures=np.asarray([1.0]), n=n, n_links=None, hist_q=np.concatenate([h, h]))
    assert st2.moments()[0][0] == q2[0]


def test_statistics_shifted_bins_return_their_centres(sg):
    # n = 10 in bins of 4: d in {0..3}, {4..7}, {8, 9, 10}: centres 1.5, 5.5, 9
    st = sg.OverlapStatistics(temperatures=np.asarray([1.0]), n=10, n_links=21, hist_q=np.ones((1, 1, 3), np.int64), q_shift=2,
                              hist_l=np.asarray([[[1, 0, 3]]], np.int64), l_shift=3)
    assert np.allclose(st.q_values(), 1.0 - 2.0 * np.asarray([1.5, 5.5, 9.0]) / 10, rtol=0, atol=1e-15)
    # L = 21 in bins of 8: b in {0..7}, {8..15}, {16..21}: centres 3.5, 11.5, 18.5
    lv = 1.0 - 2.0 * np.asarray([3.5, 11.5, 18.5]) / 21
    assert np.allclose(st.link_values(), lv, rtol=0, atol=1e-15)
    assert abs(st.link_overlap()[0] - (lv[0] + 3 * lv[2]) / 4) < 1e-15
    # fewer bins than the values need: the last bin holds the rest (the engine's clamp), up to the largest value
    st = sg.OverlapStatistics(temperatures=np.asarray([1.0]), n=10, n_links=None, hist_q=np.ones((1, 1, 2), np.int64), q_shift=1)
    assert np.allclose(st.q_values(), 1.0 - 2.0 * np.asarray([0.5, 6.0]) / 10, rtol=0, atol=1e-15)


def test_bin_shift():
    from spin_glass_anneal_rl_amd.parallel_tempering import bin_shift
    assert bin_shift(36, None) == 0 and bin_shift(36, 37) == 0 and bin_shift(36, 36) == 1
    assert bin_shift(36, 19) == 1 and bin_shift(36, 18) == 2 and bin_shift(36, 1) == 6
    assert bin_shift(2 ** 40, 4) == 31  # no shift the engine takes is enough: the last bin takes the rest


def test_parallel_tempering_configuration_checks(sg):
    Cfg, Err = sg.ParallelTemperingConfig, sg.ConfigurationError
    c = Cfg()
    assert (c.measure_overlaps, c.measure_after, c.measure_interval, c.overlap_bins) == (False, 0, 1, None)
    Cfg(n_copies=2, measure_overlaps=True)
    Cfg(n_copies=4, measure_overlaps=True, cluster_moves=True, measure_after=100, measure_interval=3, overlap_bins=64)
    for bad in (dict(measure_overlaps=True), dict(n_copies=1, measure_overlaps=True), dict(n_copies=3, measure_overlaps=True),
                dict(n_copies=2, measure_overlaps=True, measure_after=-1), dict(n_copies=2, measure_overlaps=True, measure_interval=0),
                dict(n_copies=2, measure_overlaps=True, overlap_bins=0), dict(n_copies=2, measure_overlaps=True, measure_interval=1.5)):
        with pytest.raises(Err):
            Cfg(**bad)
    # a configuration changed after it was made is checked again where it is used
    c = Cfg(n_copies=2, measure_overlaps=True)
    c.n_copies = 3
    with pytest.raises(Err):
        sg.ParallelTempering(c)
    pt = sg.ParallelTempering(Cfg(n_replicas=4, n_copies=2, measure_overlaps=True))
    assert pt.overlap_statistics is None and pt.overlap_rounds_measured == 0
