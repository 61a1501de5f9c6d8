"""The geometry of the tile kernel's plan (csrc/sga_kernels.h: row_shared_tile_plan), for the tests that need it: the
rule written out again in Python, and tests/c_abi/rs_tile_plan_rule.cpp compiled and asked."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc")
THREADS, EXTRA = 1024, 32        # RS_TILE_PLAN_THREADS, RS_TILE_PLAN_EXTRA
LDS = 80 * 1024                  # RS_TILE_PLAN_LDS: what the rule asks for
TILE_LDS = 160 * 1024 - 256      # RS_TILE_LDS_BUDGET: the last resort (32 replicas of W = 1024 stage 128 KB)


def lds_bytes(W, rg, tiles):
    """rg W words of staging, a counter per (tile of the pass, replica of the slice), the scan's words."""
    return 4 * (rg * W + rg * tiles + EXTRA)


def log_group(n, W):
    """row_shared_log_group: the by-site plan counts per (window, group of 2^l replicas, site)."""
    l = 5
    while (1 << l) < -(-n // W):
        l += 1
    return l


def runs_fit(n, W, S, R, rg):
    """16-bit run starts per (tile, slice) of a window inside the n ceil(R / 2^l) words of the by-site counts."""
    return 2 * -(-n // S) * -(-R // rg) <= 4 * -(-R // (1 << log_group(n, W))) * n


def plan(n, W, S, R):
    """(rg, tiles per pass): the largest rg whose staging and counters for all tiles fit; else ranges, smallest rg first."""
    ntiles = -(-n // S)
    for rg in (32, 16, 8, 4, 2, 1):
        if lds_bytes(W, rg, ntiles) <= LDS and runs_fit(n, W, S, R, rg):
            return rg, ntiles
    for budget in (LDS, TILE_LDS):
        for rg in (1, 2, 4, 8, 16, 32):
            if lds_bytes(W, rg, 1) <= budget and runs_fit(n, W, S, R, rg):
                return rg, min(ntiles, (budget // 4 - EXTRA - rg * W) // rg)
    return 0, 0


def build(directory, flags=()):
    exe = os.path.join(str(directory), "rs_tile_plan_rule")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", *flags,
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-I", "/opt/rocm/include",
                    os.path.join(ROOT, "tests", "c_abi", "rs_tile_plan_rule.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def ask(exe, queries):
    """[(n, W, S, R)] -> the program's header line and [(rg, tiles, lds, fit)]."""
    out = subprocess.run([exe] + [str(v) for q in queries for v in q], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == 1 + len(queries), out
    return out[0], [tuple(int(f.split("=")[1]) for f in line.split()) for line in out[1:]]
