"""Replica groups of the row-shared sweep (sga_set_replica_groups; csrc/sga_kernels.h: row_shared_groups and the carve of
the plan's scratch), what holds without a GPU: the pure rule through tests/c_abi/replica_groups_rule.cpp -- the ranges,
every group's view of cnt / ent / base / bits inside the engine's allocations and disjoint from its neighbours', its tile
plan inside its share, the default count on both sides of RS_GROUP_MIN_REPLICAS -- the setter's refusal and the version."""
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tile_plan_rule as tp  # noqa: E402
from conftest import ROOT  # noqa: E402

PROGRAM = os.path.join(ROOT, "tests", "c_abi", "replica_groups_rule.cpp")
MIN_REPLICAS, DEFAULT_MAX = 256, 2  # RS_GROUP_MIN_REPLICAS, RS_DEFAULT_MAX_GROUPS
RS = (1, 31, 32, 33, 64, 65, 70, 130, 1024)
# (n, W, S): the flagship's shape (S by the tile rule at 256 CUs), and the small shapes of tests/test_replica_groups_gpu.py
SHAPES = ((10000, 1024, 40), (300, 256, 24), (1100, 1024, 96))
# R: the default count -- two groups from 2 x 256 replicas (a last group of 255 is one too few), never four
DEFAULTS = {64: 1, 256: 1, 511: 1, 512: 2, 513: 2, 1023: 2, 1024: 2, 2048: 2, 4096: 2}


def build(directory, flags=()):
    exe = os.path.join(str(directory), "replica_groups_rule")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", *flags,
                    "-I", os.path.join(ROOT, "include"), "-I", tp.CSRC, "-I", "/opt/rocm/include", PROGRAM, "-o", exe],
                   check=True, capture_output=True)
    return exe


def ask(exe, queries):
    """[(n, W, S, R, G)] -> the header line and per query (G, fit, default, [(r0, r1, cnt, ent, base, bits, n_groups, rg, tiles)])."""
    out = subprocess.run([exe] + [str(v) for q in queries for v in q], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == 1 + len(queries), out
    got = []
    for line in out[1:]:
        head, *groups = line.split(" | ")
        G, fit, default = (int(f.split("=")[1]) for f in head.split())
        got.append((G, fit, default, [tuple(int(v) for v in g.split()) for g in groups]))
    return out[0], got


def expected_ranges(R, G):
    """The rule written out again: one group up to 32 replicas; else whole 32-replica slices dealt out evenly."""
    if R <= 32 or G <= 1:
        return [(0, R)]
    slices = -(-R // 32)
    G = min(G, 4, slices)
    b = [32 * (slices * i // G) for i in range(G)] + [R]
    return list(zip(b[:-1], b[1:]))


def check(exe):
    queries = [(n, W, S, R, G) for (n, W, S) in SHAPES for R in RS for G in (1, 2, 4)]
    queries += [(10000, 256, 40, 130, 4), (10000, 256, 40, 1024, 4)]  # 40 windows: plan groups of 64 replicas
    queries += [(10000, 1024, 40, R, 0) for R in DEFAULTS]
    head, got = ask(exe, queries)
    assert head == f"max=4 min_replicas={MIN_REPLICAS} default_max={DEFAULT_MAX}" and MIN_REPLICAS >= 64
    multi = 0
    for (n, W, S, R, G), (g, fit, default, groups) in zip(queries, got):
        where = (n, W, S, R, G)
        ranges = [(r0, r1) for r0, r1, *_ in groups]
        assert ranges == expected_ranges(R, G) and g == len(groups) <= max(G, 1), where
        # ascending, disjoint, none empty, covering [0, R); inner boundaries whole slices of 32
        assert ranges[0][0] == 0 and ranges[-1][1] == R and all(r0 < r1 for r0, r1 in ranges), where
        assert all(a[1] == b[0] and b[0] % 32 == 0 for a, b in zip(ranges, ranges[1:])), where
        if R <= 32:
            assert g == 1, where
        nwin, ntiles, l = -(-n // W), -(-n // S), tp.log_group(n, W)
        nw32 = 8 * -(-n // 256)
        alloc_groups = -(-R // (1 << l))
        shares = 0
        for i, (r0, r1, cnt, ent, base, bits, n_groups, rg, tiles) in enumerate(groups):
            Rg = r1 - r0
            assert (rg, tiles) == tp.plan(n, W, S, Rg), where
            assert (ent, base, bits) == (r0 * n, r0 * W, r0 * nw32), where  # per replica: the views tile the arrays
            assert n_groups == -(-Rg // (1 << l)) and cnt == nwin * n * shares, where
            shares += n_groups
            if g > 1 and fit:  # the group's 16-bit run starts inside its share of cnt, in bytes
                assert rg > 0 and 2 * nwin * ntiles * -(-Rg // rg) <= 4 * nwin * n * n_groups, where
        if g > 1:
            multi += 1
            assert fit == int(shares <= alloc_groups and all(grp[7] > 0 for grp in groups)), where
        else:
            assert fit == 1, where
    assert multi > 30
    by = {q: r for q, r in zip(queries, got)}
    assert [(r0, r1) for r0, r1, *_ in by[(300, 256, 24, 33, 4)][3]] == [(0, 32), (32, 33)]
    assert [(r0, r1) for r0, r1, *_ in by[(10000, 1024, 40, 1024, 4)][3]] == [(0, 256), (256, 512), (512, 768), (768, 1024)]
    # every committed shape admits its groups at every R; beyond 32 windows the shares of ranges cut at 32 round up past the
    # allocation (130 replicas in plan groups of 64: four shares against three), and the answer is one group
    for (n, W, S) in SHAPES:
        assert all(by[(n, W, S, R, G)][1] == 1 for R in RS for G in (1, 2, 4))
    assert by[(10000, 256, 40, 130, 4)][:2] == (4, 0) and by[(10000, 256, 40, 1024, 4)][:2] == (4, 1)
    # the default: the largest of RS_DEFAULT_MAX_GROUPS ... 2, 1 that leaves every group at least RS_GROUP_MIN_REPLICAS replicas
    assert {R: by[(10000, 1024, 40, R, 0)][2] for R in DEFAULTS} == DEFAULTS


def test_the_group_rule(tmp_path):
    check(build(tmp_path))


def test_the_group_rule_under_sanitizers(tmp_path):
    """The same program, stand-alone, with the address and undefined-behaviour sanitizers on its host code."""
    check(build(tmp_path, flags=("-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all")))


def test_version_and_interface():
    import spin_glass_anneal_rl_amd as sg
    L = sg._native.lib()
    assert L.sga_version() >= 2400
    header = open(os.path.join(ROOT, "include", "sga.h")).read()
    assert re.search(r"^int sga_set_replica_groups\(sga_engine \*e, int g\);", header, re.M)
    assert re.search(r"^int sga_get_replica_groups\(sga_engine \*e, int \*g\);", header, re.M)
    assert L.sga_set_replica_groups(None, 2) == sg._native.ERR_INVALID  # (an engine's refusals: tests/test_replica_groups_gpu.py)
    assert L.sga_get_replica_groups(None, None) == sg._native.ERR_INVALID
    assert callable(sg.AnnealEngine.set_replica_groups) and callable(sg.AnnealEngine.replica_groups)
