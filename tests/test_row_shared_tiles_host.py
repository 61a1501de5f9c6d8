"""Row-shared fields in tiles of sites (options "row_shared_fields", "row_shared_tile_sites"), what holds without a GPU:
the version, the two options and their place in the list, and the host rule for the tile size
(tests/c_abi/rs_tile_rule.cpp over sga_kernels.h: row_shared_tile_sites, row_shared_tile_lds)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc")
LDS = 160 * 1024 - 256  # RS_TILE_LDS_BUDGET
ENTRIES, THREADS, MAX_R = 6144, 1024, 4096


@pytest.fixture(scope="module")
def N():
    import spin_glass_anneal_rl_amd as sg
    return sg._native


def test_version_and_options(N):
    assert N.lib().sga_version() >= 1900
    names = N.option_names()
    at = names.index("row_shared_grid")
    assert names[at + 1:at + 4] == ["row_shared_fields", "row_shared_tile_sites", "row_shared_window"]
    q = N.route_query()
    assert q.opt[names.index("row_shared_fields")] == 2 and q.opt[names.index("row_shared_tile_sites")] == 0  # the defaults
    text = open(os.path.join(CSRC, "sga_route.h")).read()
    assert '{"row_shared_fields", "SGA_ROW_SHARED_FIELDS", 0, 0, 2, 0, 2, 0},' in text  # default 2, range [0, 2], [sweep]
    assert '{"row_shared_tile_sites", "SGA_ROW_SHARED_TILE_SITES", 0, 0, 0, 0, 4096, 0},' in text
    header = open(os.path.join(ROOT, "include", "sga.h")).read()
    assert re.search(r'"row_shared_fields"\s+0 \| 1 \| 2 \(default\)', header) and "[sweep; SGA_ROW_SHARED_FIELDS]" in header
    assert re.search(r'"row_shared_tile_sites"\s+0 \(default\)', header) and "[sweep; SGA_ROW_SHARED_TILE_SITES]" in header


def test_the_options_leave_the_route_alone(N):
    """Which fields kernel runs is no routing decision: sga_explain_route answers the same whatever the two options say."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "route_table.json")) as f:
        cases = json.load(f)["cases"]
    for c in cases:
        opts = dict(c["query"].get("options") or {})
        for extra in ({"row_shared_fields": 0}, {"row_shared_fields": 1, "row_shared_tile_sites": 64}):
            assert N.explain_route(N.route_query(**{**c["query"], "options": {**opts, **extra}})) == c["explain"], c["name"]


def lds_bytes(n, planes, ones, S, R):
    """The tile kernel's dynamic LDS as the kernel lays it out: S rows of (1 | planes + 1) planes of 32 ceil(n / 256)
    bytes, the entry buffer (32-bit entry + 16-bit site), R counters, S + 1 offsets, S row constants, a word per wave."""
    row = (1 if ones else planes + 1) * 32 * ((n + 255) // 256)
    return S * row + ENTRIES * 6 + 4 * (R + 2 * S + 1 + THREADS // 64)


def rule(n, planes, ones, R, cus, forced):
    """The rule as DESIGN.md 4.1h states it, written out again here."""
    if R > MAX_R:
        return 0, "more replicas than the tile kernel's 4096 LDS counters"
    if lds_bytes(n, planes, ones, 2, R) > LDS:
        return 0, "two rows' planes do not fit the tile image in LDS"
    if forced > 0:
        S = min(max(forced, 2), 4096)
        return (S, "-") if lds_bytes(n, planes, ones, S, R) <= LDS else (0, "the forced tile does not fit LDS")
    m = 1
    while True:
        S = max(2, -(-n // (m * cus)))
        if S <= 4096 and lds_bytes(n, planes, ones, S, R) <= LDS:
            return S, "-"
        m += 1


QUERIES = [
    # (n, planes, sign-only, R, CUs, forced S)
    (10000, 1, 1, 1024, 256, 0), (10000, 1, 0, 1024, 256, 0), (10000, 3, 0, 1024, 256, 0), (10000, 8, 0, 1024, 256, 0),
    (2000, 1, 1, 1024, 256, 0), (64, 1, 1, MAX_R, 256, 0), (64, 1, 1, MAX_R + 1, 256, 0), (3, 1, 1, 5, 256, 0),
    (32768, 1, 1, 64, 256, 0), (32768, 8, 0, 64, 256, 0), (100000, 8, 0, 8, 256, 0), (300000, 1, 1, 8, 256, 0),
    (10000, 1, 1, 1024, 256, 80), (10000, 1, 1, 1024, 256, 200), (300, 3, 0, 5, 256, 1), (300, 3, 0, 5, 256, 64),
    (10000, 1, 1, 1024, 304, 0), (10000, 1, 1, 1024, 64, 0), (1000, 1, 0, 3, 256, 5000),
]


def takes_tiles_by_default(n, planes, ones):
    """Option "row_shared_fields" = 2: sign-only rows, a replica's spin bits (32 ceil(n / 256) bytes) from 1 KB up to the
    2 KB a quarter wave keeps in registers -- the configuration DESIGN.md 7 measured to win."""
    return bool(ones) and planes == 1 and 1024 <= 32 * ((n + 255) // 256) <= 2048


def test_tile_rule(tmp_path):
    exe = str(tmp_path / "rs_tile_rule")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "c_abi", "rs_tile_rule.cpp"), "-o", exe],
                   check=True, capture_output=True)
    args = [str(v) for q in QUERIES for v in q]
    out = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == f"threads={THREADS} entries={ENTRIES} max_replicas={MAX_R} max_sites=4096 budget={LDS}"
    assert len(out) == 1 + len(QUERIES)
    for line, q in zip(out[1:], QUERIES):
        S, why = rule(*q)
        dflt = int(S > 0 and takes_tiles_by_default(q[0], q[1], q[2]))
        assert line == f"S={S} lds={lds_bytes(q[0], q[1], q[2], S, q[3]) if S else 0} why={why} dflt={dflt}", (q, line)
    # the flagship (C2a, +-1 couplings: sign-only rows) runs 250 tiles of 40 sites on 256 CUs, one workgroup each
    assert out[1].startswith("S=40 ") and -(-10000 // 40) == 250
    # a tile of the general one-plane form holds twice the bytes per site: the same S still fits
    assert out[2].startswith("S=40 ")
    # the default takes the tiles for the flagship alone of the first five: not for general planes, not at n = 2000
    assert [ln.rsplit("dflt=", 1)[1] for ln in out[1:6]] == ["1", "0", "0", "0", "0"]
