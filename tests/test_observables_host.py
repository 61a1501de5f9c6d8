"""Replica observables (sga_get_magnetizations / sga_get_overlaps / sga_get_overlaps_with, csrc/observables.hip), what
holds without a GPU: the version, the three symbols in the library, the header and the binding, that the calls added no
option and no query field, the product's launch geometry against the rule written out again here, and the greedy rule
of AnnealEngine.distinct_best restated in numpy (tests/test_observables_gpu.py holds the engine against it)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_sequential_windows_host import OPTIONS, ROUTE_QUERY_BYTES

CSRC = os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc")
TILE, GRAIN, KMIN = 128, 128, 512  # OBS_TILE, OBS_K_GRAIN, OBS_K_MIN
CUS = 256                          # compute units of the MI355X: what the engine passes

PLAN_N = (1, 63, 64, 65, 1000, 10_000, 70_001, 1_000_000)
PLAN_ROWS = (1, 3, 17, 33, 1024)
# queries (n, rows_a, rows_b) that tests/test_observables_gpu.py runs: the K-split case and a one-range case
GPU_QUERY_SPLIT = (70_001, 5, 5)
GPU_QUERY_ONE_RANGE = (64, 17, 17)


def plan(n, rows_a, rows_b, cus):
    """observables_plan: about two workgroups per compute unit, no K range shorter than KMIN columns, ranges whole grains."""
    tiles_m, tiles_n = -(-rows_a // TILE), -(-rows_b // TILE)
    tiles = tiles_m * tiles_n
    s = min(-(-2 * cus // tiles), -(-n // KMIN))
    per = -(-n // s)
    kchunk = -(-per // GRAIN) * GRAIN
    return tiles_m, tiles_n, -(-n // kchunk), kchunk


def greedy_distinct(energies, configs, k, min_hamming=1, up_to_global_flip=False):
    """distinct_best's rule on host arrays: walk by energy ascending (ties by index), keep a configuration at least
    min_hamming away -- (n - Q) / 2, or (n - |Q|) / 2 up to a global flip -- from every one kept so far."""
    kept = []
    for r in sorted(range(len(energies)), key=lambda i: (energies[i], i)):
        if len(kept) >= k:
            break
        s = np.asarray(configs[r], np.int64)
        far = True
        for j in kept:
            q = int(s @ np.asarray(configs[j], np.int64))
            if (s.size - (abs(q) if up_to_global_flip else q)) // 2 < min_hamming:
                far = False
        if far:
            kept.append(r)
    return kept


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("observables_plan")), "observables_plan")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-I", "/opt/rocm/include",
                    os.path.join(ROOT, "tests", "c_abi", "observables_plan.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def ask(exe, queries):
    """[(n, rows_a, rows_b, cus)] -> the program's header line and [(tiles_m, tiles_n, ksplit, kchunk)]."""
    out = subprocess.run([exe] + [str(v) for q in queries for v in q], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == 1 + len(queries), out
    return out[0], [tuple(int(f.split("=")[1]) for f in line.split()) for line in out[1:]]


def test_version(sg):
    assert sg._native.lib().sga_version() >= 2300


def test_the_three_symbols_are_exported_declared_and_bound(sg):
    L, N = sg._native.lib(), sg._native
    with open(os.path.join(ROOT, "include", "sga.h")) as f:
        header = f.read()
    names = [s[0] for s in N.SYMBOLS]
    for name in ("sga_get_magnetizations", "sga_get_overlaps", "sga_get_overlaps_with"):
        assert hasattr(L, name), name
        assert name in names, name
    assert re.search(r"^int sga_get_magnetizations\(sga_engine \*e, int which, int32_t \*out", header, re.M)
    assert re.search(r"^int sga_get_overlaps\(sga_engine \*e, int which_a, int which_b, int32_t \*out, int64_t ldq", header, re.M)
    assert re.search(r"^int sga_get_overlaps_with\(sga_engine \*e, int which, const int8_t \*cfg, int64_t ld", header, re.M)
    assert re.search(r"^#define SGA_SPINS_CURRENT 0\b", header, re.M) and re.search(r"^#define SGA_SPINS_BEST +1\b", header, re.M)
    assert (N.SPINS_CURRENT, N.SPINS_BEST) == (0, 1)
    # a NULL engine is an error, not a crash (no device is touched)
    out = (ctypes.c_int32 * 4)()
    cfg = (ctypes.c_int8 * 4)(1, 1, 1, 1)
    assert L.sga_get_magnetizations(None, 0, out) == N.ERR_INVALID
    assert L.sga_get_overlaps(None, 0, 0, out, 2) == N.ERR_INVALID
    assert L.sga_get_overlaps_with(None, 0, cfg, 4, 1, out, 1) == N.ERR_INVALID


def test_no_option_and_no_query_field_was_added(sg):
    N = sg._native
    assert N.option_names() == OPTIONS
    assert ctypes.sizeof(N.RouteQuery) == ROUTE_QUERY_BYTES


def test_the_plan_is_the_rule_and_covers_the_product_once(plan_exe):
    queries = [(n, ra, rb, cus) for cus in (CUS, 64) for n in PLAN_N for ra in PLAN_ROWS for rb in PLAN_ROWS]
    queries += [GPU_QUERY_SPLIT + (CUS,), GPU_QUERY_ONE_RANGE + (CUS,)]
    header, answers = ask(plan_exe, queries)
    assert header == f"tile={TILE} grain={GRAIN} kmin={KMIN}"
    for q, got in zip(queries, answers):
        n, ra, rb, cus = q
        assert got == plan(*q), q
        tiles_m, tiles_n, ksplit, kchunk = got
        # K ranges [s kchunk, min(n, (s + 1) kchunk)): none empty, together [0, n) once; whole grains, so that every
        # range starts on a 16-byte boundary of its row
        assert ksplit >= 1 and kchunk % GRAIN == 0, q
        edges = [min(n, s * kchunk) for s in range(ksplit + 1)]
        assert edges[0] == 0 and edges[-1] == n and all(a < b for a, b in zip(edges, edges[1:])), q
        # tiles of TILE rows: none empty, together rows_a x rows_b once
        for tiles, rows in ((tiles_m, ra), (tiles_n, rb)):
            assert (tiles - 1) * TILE < rows <= tiles * TILE, q
    by_query = dict(zip(queries, answers))
    assert by_query[GPU_QUERY_SPLIT + (CUS,)][2] >= 3
    assert by_query[GPU_QUERY_ONE_RANGE + (CUS,)][2] == 1
    # the flagship shape fills the chip: 64 tiles (36 computed where A is B) in 8 ranges
    assert by_query[(10_000, 1024, 1024, CUS)] == (8, 8, 8, 1280)


def test_greedy_rule_two_identical_bests():
    a = np.array([1, -1, 1, 1, -1, 1], np.int8)
    b = np.array([1, 1, 1, -1, -1, 1], np.int8)
    assert greedy_distinct([-3.0, -3.0, -2.0], [a, a.copy(), b], 3) == [0, 2]
    assert greedy_distinct([-3.0, -3.0, -2.0], [a, a.copy(), b], 3, min_hamming=0) == [0, 1, 2]
    assert greedy_distinct([-3.0, -3.0, -2.0], [a, a.copy(), b], 3, min_hamming=3) == [0]  # (b is 2 flips from a)
    assert greedy_distinct([-3.0, -3.0, -2.0], [a, a.copy(), b], 1) == [0]


def test_greedy_rule_global_flip():
    a = np.array([1, -1, 1, 1, -1, 1, 1], np.int8)
    c = a.copy()
    c[0] = -c[0]
    configs, energies = [a, -a, c], [-5.0, -5.0, -4.0]
    assert greedy_distinct(energies, configs, 3) == [0, 1, 2]
    assert greedy_distinct(energies, configs, 3, up_to_global_flip=True) == [0, 2]
    assert greedy_distinct(energies, configs, 3, min_hamming=2, up_to_global_flip=True) == [0]
    # n odd: Q is odd, (n - |Q|) / 2 is a whole number of flips
    assert greedy_distinct(energies, [a, -c, c], 3, up_to_global_flip=True) == [0, 1]  # (-c is one flip from -a; c is -(-c))


def test_greedy_rule_tie_in_energy():
    a = np.array([1, 1, 1, 1], np.int8)
    b = np.array([1, 1, -1, -1], np.int8)
    c = np.array([-1, 1, -1, 1], np.int8)
    # equal energies go by replica index, whatever the order of the configurations
    assert greedy_distinct([-1.0, -2.0, -2.0], [a, b, c], 2) == [1, 2]
    assert greedy_distinct([-2.0, -1.0, -2.0], [a, b, c], 2) == [0, 2]
    assert greedy_distinct([-2.0, -2.0, -2.0], [c, b, a], 3) == [0, 1, 2]
