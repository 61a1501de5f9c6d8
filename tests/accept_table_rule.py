"""The chain's accept table (csrc/sga_kernels.h: rs_accept_table_entries; csrc/sweep_dense_rs.hip: rs_accept_tabled), for
the tests that need it: the rule written out again in Python, the decision in its table form and in the direct form of
rs_accept with the oracle's expf, and tests/c_abi/rs_accept_table_rule.cpp compiled and asked."""
import math
import os
import subprocess

import numpy as np

import oracle
from conftest import ROOT

CSRC = os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc")
MAX = 1023           # RS_ACCEPT_TABLE_MAX
NO_BOUND = 2 ** 31 - 1


def zero_from(T):
    """floor(52 T) + 2 where 0 <= 52 T < 1023 (the product rounded as fp64 rounds it), else no bound."""
    x = 52.0 * T
    return int(math.floor(x)) + 2 if 0.0 <= x < MAX else NO_BOUND


def entries(T, table_m):
    """Q = min(table_m, 1023, floor(52 T) + 2)."""
    return min(max(min(table_m, MAX), 0), zero_from(T))


def probability(q, T):
    """expf_det((float)(-(double)(2 q) / T)), q >= 1: the expression of rs_accept."""
    with np.errstate(divide="ignore"):
        return oracle.expf(np.float32(-np.float64(2 * q) / np.float64(T)))


def direct(q, u, T, table_m):
    """rs_accept on fk = q."""
    if q <= 0:
        return True
    if q <= table_m:
        return u < probability(q, T)
    return False if 2.0 * q > T * 104.0 else u < probability(q, T)


def tabled(q, u, T, table_m):
    """rs_accept_tabled on fk = q -> (decision, how: 'table' | 'zero' | 'lane' | 'down')."""
    if q <= 0:
        return True, "down"
    Q = entries(T, table_m)
    if q <= Q:
        return u < probability(q, T), "table"
    if Q == zero_from(T):
        return False, "zero"
    return direct(q, u, T, table_m), "lane"


def build(directory, flags=()):
    exe = os.path.join(str(directory), "rs_accept_table_rule")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", *flags,
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-I", "/opt/rocm/include",
                    os.path.join(ROOT, "tests", "c_abi", "rs_accept_table_rule.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def ask(exe, queries):
    """[(T, table_m)] -> the program's header line and [(Q, zero_from)]."""
    args = [w for T, m in queries for w in (float(T).hex() if math.isfinite(T) else "inf", str(m))]
    out = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == 1 + len(queries), out
    return out[0], [tuple(int(f.split("=")[1]) for f in line.split()) for line in out[1:]]
