"""Class-resolved overlaps between pairs of replicas (sga_get_class_overlaps / sga_accumulate_ladder_class_overlaps,
csrc/class_overlaps.hip), what holds without a GPU: the version, the two symbols in the library, the header and the
binding, that the calls added no option and no query field, the reference of tests/class_overlap_reference.py against
cases worked out by hand, the kernel's counter copies, LDS bytes, bound and argument checks
(tests/c_abi/class_overlaps_plan.cpp), lattice_planes, ClassOverlapStatistics on sums known in closed form, and the
configuration checks of ParallelTemperingConfig (tests/test_class_overlaps_gpu.py holds the engine against the reference)."""
import ctypes
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import class_overlap_reference as cor
from conftest import ROOT
from test_sequential_windows_host import OPTIONS, ROUTE_QUERY_BYTES

CSRC = os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc")


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("class_overlaps_plan")), "class_overlaps_plan")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-I", "/opt/rocm/include",
                    os.path.join(ROOT, "tests", "c_abi", "class_overlaps_plan.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def plan(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.strip()


def test_version(sg):
    assert sg._native.lib().sga_version() >= 2800


def test_the_two_symbols_are_exported_declared_and_bound(sg):
    L, N = sg._native.lib(), sg._native
    with open(os.path.join(ROOT, "include", "sga.h")) as f:
        header = f.read()
    names = [s[0] for s in N.SYMBOLS]
    for name in ("sga_get_class_overlaps", "sga_accumulate_ladder_class_overlaps"):
        assert hasattr(L, name), name
        assert name in names, name
    assert re.search(r"^int sga_get_class_overlaps\(sga_engine \*e, int which[^;]*const int32_t \*pairs[^;]*int count,\s+"
                     r"const int32_t \*classes[^;]*int64_t ld, int n_maps, int n_classes,\s+int32_t \*dist[^;]*\);", header, re.M)
    assert re.search(r"^int sga_accumulate_ladder_class_overlaps\(sga_engine \*e, int slot_lo, int slot_hi,\s+"
                     r"const int32_t \*classes[^;]*int64_t ld, int n_maps, int n_classes,\s+uint64_t \*sum1, uint64_t \*sum2[^;]*\);",
                     header, re.M)
    assert "a run keeps its map on the device" in header        # a host map is staged on every call
    assert "measurements (max_c N_c)^2 < 2^64" in header         # the overflow bound is the caller's
    for name in ("class_overlaps", "accumulate_ladder_class_overlaps"):
        assert hasattr(sg.AnnealEngine, name), name
    assert hasattr(sg, "ClassOverlapStatistics") and hasattr(sg.encoders, "lattice_planes")


def test_no_option_and_no_query_field_was_added(sg):
    N = sg._native
    assert N.option_names() == OPTIONS
    assert ctypes.sizeof(N.RouteQuery) == ROUTE_QUERY_BYTES


# ---- the reference, against cases worked out by hand -------------------------------------------------------------------
def test_reference_arcs_of_a_ring():
    n = 12
    classes = np.arange(n) // 4  # classes {0..3}, {4..7}, {8..11}
    s_a = np.ones(n, np.int8)
    s_b = s_a.copy()
    s_b[[2, 3, 4, 8, 9, 11, 0]] = -1  # arcs {2, 3, 4}, {8, 9} and, through the ring's closing bond, {11, 0}
    D = cor.class_dist(s_a, s_b, classes, 3)
    assert D.dtype == np.int32 and D.tolist() == [[3, 1, 3]]  # {0, 2, 3}, {4}, {8, 9, 11}
    assert D.sum() == 7
    assert cor.class_dist(s_a, s_a, classes, 3).tolist() == [[0, 0, 0]]
    assert cor.class_dist(s_a, -s_a, classes, 3).tolist() == [[4, 4, 4]]  # every site differs: D_c = N_c


def test_reference_values_outside_the_range_are_no_class():
    classes = np.asarray([0, -1, 1, 2, 1, 0, -7, 2], np.int32)  # n_classes = 2: -1, -7 and the two 2s are no class
    s_a = np.ones(8, np.int8)
    D = cor.class_dist(s_a, -s_a, classes, 2)
    assert D.tolist() == [[2, 2]] and D.sum() == 4  # four of the eight differing sites are masked
    s_b = s_a.copy()
    s_b[[1, 3, 6]] = -1  # only masked sites differ
    assert cor.class_dist(s_a, s_b, classes, 2).tolist() == [[0, 0]]


def test_reference_two_maps_at_once_and_the_pair_form():
    classes = np.asarray([[0, 0, 1, 1, 2, 2], [0, 1, 0, 1, 0, 1]], np.int32)
    S = np.asarray([[1, 1, 1, 1, 1, 1], [-1, 1, 1, -1, -1, -1], [1, 1, 1, 1, 1, 1]], np.int8)
    out = cor.pair_form(S, [(0, 1), (1, 1), (0, 2), (1, 2)], classes, 3)
    assert out.shape == (4, 2, 3) and out.dtype == np.int32
    assert out[0].tolist() == [[1, 1, 2], [2, 2, 0]]  # sites 0, 3, 4, 5 differ
    assert out[1].tolist() == [[0, 0, 0], [0, 0, 0]] and out[2].tolist() == out[1].tolist()
    assert np.array_equal(out[3], out[0])


def test_reference_accumulate():
    classes = np.asarray([0, 0, 1, 1], np.int32)
    S = np.asarray([[1, 1, 1, 1], [1, -1, 1, 1], [-1, -1, -1, -1], [1, 1, -1, -1]], np.int8)
    s1, s2 = np.zeros((1, 2, 1, 2), np.uint64), np.zeros((1, 2, 1, 2, 2), np.uint64)
    # two ladders of two slots; slot 0: replicas 1 and 2 (D = 1, 2), slot 1: replicas 0 and 3 (D = 0, 2)
    for _ in range(2):
        cor.accumulate(s1, s2, [1, 0, 2, 3], 2, S, classes, 2)
    assert s1[0, :, 0].tolist() == [[2, 4], [0, 4]]
    assert s2[0, 0, 0].tolist() == [[2, 4], [4, 8]] and s2[0, 1, 0].tolist() == [[0, 0], [0, 8]]
    s1r = np.zeros((1, 1, 1, 2), np.uint64)
    cor.accumulate(s1r, None, [1, 0, 2, 3], 2, S, classes, 2, slot_lo=1, slot_hi=2)
    assert s1r[0, 0, 0].tolist() == [0, 2]


# ---- the kernel's host half ------------------------------------------------------------------------------------------
def test_copies_lds_bytes_and_the_bound(plan_exe):
    mcs = [1, cor.MAX_MC_4, cor.MAX_MC_4 + 1, cor.MAX_MC, cor.MAX_MC + 1]
    out = plan(plan_exe, "lds", *mcs).split("\n")
    assert out[0].split() == [f"budget={cor.LDS_BUDGET}", f"max_mc={cor.MAX_MC}", f"max_mc_4={cor.MAX_MC_4}", "threads=256"]
    got = [tuple(int(v) for v in line.split()) for line in out[1:]]
    assert got[:4] == [(cor.copies(mc), cor.lds_bytes(mc)) for mc in mcs[:4]]
    assert got[0] == (4, 16)                                   # one counter, a copy a wave
    assert got[1] == (4, 16 * 10224) and got[1][1] <= cor.LDS_BUDGET < 16 * 10225  # the largest product with four copies
    assert got[2] == (1, 4 * 10225)                            # one more: the waves share one copy
    assert got[3] == (1, 4 * 40896) and got[3][1] <= cor.LDS_BUDGET  # at the bound
    assert got[4][1] > cor.LDS_BUDGET                          # one more would not fit: the argument check refuses it
    assert (cor.MAX_MC_4, cor.MAX_MC) == (10224, 40896)


def test_every_argument_check(plan_exe):
    a = lambda *v: plan(plan_exe, "args", *v)  # noqa: E731  have_classes have_out n_maps n_classes ld n
    assert a(1, 1, 1, 1, 1, 1) == "ok" and a(1, 1, 3, 22, 10648, 10648) == "ok" and a(1, 1, 2, 5, 40, 33) == "ok"
    assert a(0, 1, 1, 1, 1, 1) == "invalid: classes is NULL"
    assert a(1, 0, 1, 1, 1, 1) == "invalid: the output is NULL"
    assert "n_maps" in a(1, 1, 0, 4, 8, 8) and "n_maps" in a(1, 1, -1, 4, 8, 8)
    assert "n_classes" in a(1, 1, 1, 0, 8, 8) and "n_classes" in a(1, 1, 1, -3, 8, 8)
    assert a(1, 1, 1, 4, 7, 8) == "invalid: ld is smaller than n" and a(1, 1, 1, 4, 8, 8) == "ok"
    assert a(1, 1, 1, cor.MAX_MC, 8, 8) == "ok" and a(1, 1, 2, cor.MAX_MC // 2, 8, 8) == "ok"
    assert a(1, 1, 1, cor.MAX_MC + 1, 8, 8).startswith("unsupported: ") and "40896" in a(1, 1, 1, cor.MAX_MC + 1, 8, 8)
    assert a(1, 1, 3, cor.MAX_MC // 3 + 1, 8, 8).startswith("unsupported: ")
    assert a(1, 1, 65536, 65536, 8, 8).startswith("unsupported: ")  # the product is formed in 64 bits
    assert a(1, 1, 1, cor.MAX_MC + 1, 7, 8).startswith("invalid: ")  # what is invalid is said first


# ---- lattice_planes --------------------------------------------------------------------------------------------------
def test_lattice_planes(sg):
    P = sg.encoders.lattice_planes((2, 3, 4))
    assert P.dtype == np.int32 and P.shape == (3, 24)
    for i, (x, y, z) in enumerate(itertools.product(range(2), range(3), range(4))):  # row-major: the last axis the fastest
        assert P[:, i].tolist() == [x, y, z]
    assert np.array_equal(sg.encoders.lattice_planes((5,)), np.arange(5, dtype=np.int32).reshape(1, 5))
    with pytest.raises(ValueError):
        sg.encoders.lattice_planes((3, 0))


# ---- ClassOverlapStatistics on sums known in closed form ---------------------------------------------------------------
def sums(measured, C):
    """sum1 [1, 1, 1, C] and sum2 [1, 1, 1, C, C] of a list of D vectors, in exact integers."""
    D = np.asarray(measured, np.uint64).reshape(-1, C)
    return D.sum(0).reshape(1, 1, 1, C), (D[:, :, None] * D[:, None, :]).sum(0).reshape(1, 1, 1, C, C)


def test_statistics_identical_copies(sg):
    C, N, T = 4, 8, 5
    s1, s2 = sums(np.zeros((T, C)), C)  # every measurement D = 0: Q_c = N_c
    st = sg.ClassOverlapStatistics(temperatures=np.asarray([1.0]), class_sizes=np.full((1, C), N), measurements=T, sum1=s1, sum2=s2)
    assert np.array_equal(st.class_correlations(), np.full((1, 1, 1, C, C), float(N * N)))
    assert st.susceptibility(0.0).tolist() == [float(C * N)]  # (sum_c N_c)^2 / n = n
    assert abs(st.susceptibility(2 * math.pi / C)[0]) < 1e-12 * C * N
    assert np.isposinf(st.correlation_length()[0])  # chi(k_min) = 0 < chi(0): +inf, as documented


def test_statistics_a_cosine_profile_has_no_k0_component(sg):
    C, N, A = 4, 8, 4
    Q = np.asarray([A, 0, -A, 0])  # A cos(2 pi c / C), exact in integers
    s1, s2 = sums([(N - Q) // 2], C)
    st = sg.ClassOverlapStatistics(temperatures=np.asarray([1.0]), class_sizes=np.full((1, C), N), measurements=1, sum1=s1, sum2=s2)
    assert np.array_equal(st.class_correlations()[0, 0, 0], np.outer(Q, Q).astype(np.float64))
    assert st.susceptibility(0.0)[0] == 0.0                      # (sum_c Q_c)^2 = 0
    assert abs(st.susceptibility(2 * math.pi / C)[0] - (2 * A) ** 2 / (C * N)) < 1e-12  # |sum_c Q_c e^{ikc}|^2 / n
    assert np.isnan(st.correlation_length()[0])                  # the radicand is -1


def test_statistics_independent_planes(sg):
    C, N = 4, 4
    # every pattern Q_c = +-2 once: <Q_c Q_c'> = 4 delta_cc'
    s1, s2 = sums([[(N - q) // 2 for q in Q] for Q in itertools.product((-2, 2), repeat=C)], C)
    assert s1.reshape(-1).tolist() == [32] * 4 and s2[0, 0, 0, 0].tolist() == [80, 64, 64, 64]
    st = sg.ClassOverlapStatistics(temperatures=np.asarray([1.0]), class_sizes=np.full((1, C), N), measurements=2 ** C, sum1=s1, sum2=s2)
    assert np.array_equal(st.class_correlations()[0, 0, 0], 4.0 * np.eye(C))
    for k in (0.0, 2 * math.pi / C, 1.234, math.pi):
        assert st.susceptibility(k)[0] == 1.0  # C v / n with v = 4: flat in k
    assert st.correlation_length()[0] == 0.0


def test_statistics_averages_maps_and_pairs_and_knows_nothing_measured(sg):
    C, N = 4, 4
    s1, s2 = sums([[(N - q) // 2 for q in Q] for Q in itertools.product((-2, 2), repeat=C)], C)
    z1, z2 = np.zeros_like(s1), np.zeros_like(s2)  # a second pair and map that never differ: <Q_c Q_c'> = 16
    S1 = np.stack([np.concatenate([s1, z1], 2), np.concatenate([z1, s1], 2)]).reshape(2, 1, 2, C)
    S2 = np.stack([np.concatenate([s2, z2], 2), np.concatenate([z2, s2], 2)]).reshape(2, 1, 2, C, C)
    st = sg.ClassOverlapStatistics(temperatures=np.asarray([1.0]), class_sizes=np.full((2, C), N), measurements=16, sum1=S1, sum2=S2)
    assert st.class_correlations().shape == (2, 1, 2, C, C)
    assert st.susceptibility(0.0)[0] == 0.5 * (1.0 + 16.0)  # the mean of chi(0) = 1 and chi(0) = n = 16
    none = sg.ClassOverlapStatistics(temperatures=np.asarray([1.0]), class_sizes=np.full((1, C), N), measurements=0, sum1=z1, sum2=z2)
    assert np.isnan(none.class_correlations()).all() and np.isnan(none.correlation_length()[0])
    with pytest.raises(sg.ConfigurationError):
        sg.ClassOverlapStatistics(temperatures=np.asarray([1.0]), class_sizes=np.full((1, C), N), measurements=1, sum1=z1).class_correlations()


def test_statistics_large_sums_are_formed_in_integers(sg):
    # N_c = 2^26 and T = 2^9 measurements of D = N_c / 2 - 1: Q_c = 2, and T N_c^2 = 2^61 is far past float64's integers
    N, T, C = 2 ** 26, 2 ** 9, 2
    D = N // 2 - 1
    s1 = np.full((1, 1, 1, C), T * D, np.uint64)
    s2 = np.full((1, 1, 1, C, C), T * D * D, np.uint64)
    st = sg.ClassOverlapStatistics(temperatures=np.asarray([1.0]), class_sizes=np.full((1, C), N), measurements=T, sum1=s1, sum2=s2)
    assert np.array_equal(st.class_correlations()[0, 0, 0], np.full((C, C), 4.0))


# ---- configuration ---------------------------------------------------------------------------------------------------
def test_parallel_tempering_configuration_checks(sg):
    Cfg, Err = sg.ParallelTemperingConfig, sg.ConfigurationError
    c = Cfg()
    assert (c.measure_class_overlaps, c.overlap_classes) == (False, None)
    planes = sg.encoders.lattice_planes((2, 2, 2))
    Cfg(n_copies=2, measure_class_overlaps=True, overlap_classes=planes)
    Cfg(n_copies=4, measure_class_overlaps=True, overlap_classes=planes[0], measure_overlaps=True, cluster_moves=True, measure_after=10)
    Cfg(overlap_classes=planes)  # a map without the flag is carried, not used
    for bad in (dict(measure_class_overlaps=True, overlap_classes=planes), dict(n_copies=3, measure_class_overlaps=True, overlap_classes=planes),
                dict(n_copies=2, measure_class_overlaps=True), dict(n_copies=2, measure_class_overlaps=True, overlap_classes=planes.astype(np.float32)),
                dict(n_copies=2, measure_class_overlaps=True, overlap_classes=np.zeros((2, 2, 2), np.int32)),
                dict(n_copies=2, measure_class_overlaps=True, overlap_classes=np.full(8, -1)),
                dict(n_copies=2, measure_class_overlaps=True, overlap_classes=np.zeros(0, np.int32)),
                dict(n_copies=2, measure_class_overlaps=True, overlap_classes=planes, measure_interval=0)):
        with pytest.raises(Err):
            Cfg(**bad)
    pt = sg.ParallelTempering(Cfg(n_replicas=4, n_sweeps=100, exchange_interval=10, n_copies=2, measure_class_overlaps=True,
                                  overlap_classes=planes, measure_after=25, measure_interval=2))
    assert pt.class_overlap_statistics is None
    cl, n_classes, sizes, planned = pt.class_overlap_plan(8)
    assert cl.dtype == np.int32 and cl.shape == (3, 8) and n_classes == 2 and np.array_equal(sizes, np.full((3, 2), 4))
    assert planned == 4  # rounds behind sweeps 10 ... 90; from 30 on (31 >= 25) seven, every second one: 30, 50, 70, 90
    with pytest.raises(Err):
        pt.class_overlap_plan(9)  # the map is not the model's


def test_planned_measurements():
    from spin_glass_anneal_rl_amd.parallel_tempering import planned_measurements
    for ns, ei, after, every in itertools.product((1, 2, 9, 10, 11, 37), (1, 2, 5, 10), (0, 1, 3, 10, 11, 12, 40), (1, 2, 3)):
        eligible = [s for s in range(1, ns) if s % ei == 0 and s + 1 >= after]
        assert planned_measurements(ns, ei, after, every) == len(eligible[::every]), (ns, ei, after, every)


def test_the_run_refuses_sums_that_could_overflow(sg):
    Cfg, Err = sg.ParallelTemperingConfig, sg.ConfigurationError
    n = 2 ** 22
    one_class = np.zeros(n, np.int32)  # N_c^2 = 2^44: 2^19 measurements reach 2^63
    ok = sg.ParallelTempering(Cfg(n_replicas=2, n_sweeps=2 ** 19, exchange_interval=1, n_copies=2, measure_class_overlaps=True,
                                  overlap_classes=one_class))
    assert ok.class_overlap_plan(n)[3] == 2 ** 19 - 1
    bad = sg.ParallelTempering(Cfg(n_replicas=2, n_sweeps=2 ** 19 + 1, exchange_interval=1, n_copies=2, measure_class_overlaps=True,
                                   overlap_classes=one_class))
    with pytest.raises(Err, match="overflow"):
        bad.class_overlap_plan(n)
    half = np.arange(n, dtype=np.int32) % 2  # two classes of 2^21: four times the room
    assert sg.ParallelTempering(Cfg(n_replicas=2, n_sweeps=2 ** 21, exchange_interval=1, n_copies=2, measure_class_overlaps=True,
                                    overlap_classes=half)).class_overlap_plan(n)[3] == 2 ** 21 - 1
    with pytest.raises(Err, match="overflow"):
        sg.ParallelTempering(Cfg(n_replicas=2, n_sweeps=2 ** 21 + 1, exchange_interval=1, n_copies=2, measure_class_overlaps=True,
                                 overlap_classes=half)).class_overlap_plan(n)
    # run() makes the same check before it touches the device
    model = type("Model", (), {"n_spins": n, "device": "cpu"})()
    with pytest.raises(Err, match="overflow"):
        bad.run(model)
