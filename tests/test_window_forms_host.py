"""The window forms' admission rules (csrc/sga_windows.h, the pure half) without a GPU, through tests/c_abi/window_forms.cpp:
against the answers of the commit before the module existed (tests/golden/window_forms.json), by hand at every threshold
of the documented rules, against sga_explain_route over the dense cases of the route table, under the sanitizers as a
stand-alone program -- and the three resets of the forms' state (tests/c_abi/window_state.cpp)."""
import json
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HOST = ["-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-I", "/opt/rocm/include"]
METROPOLIS, GLAUBER, HEAT_BATH, WOLFF = 0, 1, 2, 3

# A problem both forms take in every class below: 1000 spins, 64 replicas, padded strides, option "row_shared" = 1, windows of
# 512 for sequential sweeps, resident planes and the tiles forced (option "row_shared_fields" = 1).
COMMON = dict(dense=1, implicit=0, ragged=0, n_models=1, shared_j=0, n=1000, R=64, ldj=1024, sstride=1024, want_i8=0, acc64=0,
              table_m=2048, j_abs_max=1, grid_planes=0, grid_k=0, consistent_dE=1, packed=1, rule=METROPOLIS, field_cache=0,
              cus=256, row_shared=1, row_shared_grid=0, row_shared_window=0, row_shared_fields=1, row_shared_tile_sites=0,
              look_ahead=1, force_general=0, tuned_w=0, tuned_rule=METROPOLIS, suspend=0, seq_w=512, planes_resident=1, ones=0,
              tiles_refused=0, lean=1)


def bases():
    """A base case per class: the integer class at |J| <= 1 | 7 | 255, the grid with 1 | 3 | 8 planes at k = 0 | 2; fp32 and int8 rows."""
    out = {}
    for i8 in (0, 1):
        rows = "i8" if i8 else "f32"
        for j in (1, 7, 255):
            out[f"int-j{j}-{rows}"] = dict(COMMON, want_i8=i8, j_abs_max=j)
        for planes in (1, 3, 8):
            for k in (0, 2):
                out[f"grid-p{planes}-k{k}-{rows}"] = dict(COMMON, want_i8=i8, table_m=0, row_shared_grid=1, grid_planes=planes, grid_k=k)
    return out


# every admission trait flipped alone, the traits of each form's own remainder, the tiles' -- then a few together
FLIPS = [
    {}, {"dense": 0}, {"dense": 0, "implicit": 1}, {"ragged": 1}, {"n_models": 3}, {"n_models": 3, "shared_j": 1}, {"consistent_dE": 0},
    {"packed": 0}, {"rule": GLAUBER}, {"rule": HEAT_BATH}, {"rule": WOLFF}, {"field_cache": 1}, {"field_cache": 2}, {"force_general": 1},
    {"look_ahead": 0}, {"row_shared": 0}, {"row_shared": 2}, {"suspend": 1}, {"lean": 0}, {"acc64": 1}, {"table_m": 0}, {"table_m": 2048},
    {"row_shared_grid": 0}, {"row_shared_grid": 1}, {"grid_planes": 0}, {"grid_planes": 3, "grid_k": 1}, {"j_abs_max": 256},
    {"j_abs_max": 127}, {"j_abs_max": 128}, {"R": (1 << 20) - 1}, {"R": 1 << 20}, {"R": 0}, {"n": 0},
    {"n": 100000, "R": 30000, "ldj": 100096, "sstride": 100096}, {"seq_w": 0}, {"seq_w": 1024}, {"sstride": 1000}, {"sstride": 992},
    {"ldj": 992}, {"row_shared_window": 256}, {"row_shared_window": 512}, {"row_shared_window": 1024}, {"tuned_w": 256},
    {"tuned_w": 256, "tuned_rule": GLAUBER}, {"row_shared_fields": 0}, {"row_shared_fields": 2}, {"ones": 1}, {"tiles_refused": 1},
    {"planes_resident": 0}, {"row_shared_tile_sites": 64}, {"R": 5000}, {"cus": 304},
    # together
    {"row_shared": 2, "tuned_w": 512}, {"row_shared": 2, "tuned_w": 512, "rule": GLAUBER},
    {"row_shared": 2, "tuned_w": 512, "rule": GLAUBER, "tuned_rule": GLAUBER}, {"row_shared_window": 300, "tuned_w": 512},
    {"acc64": 1, "row_shared_grid": 1, "grid_planes": 3, "grid_k": 1}, {"row_shared": 0, "look_ahead": 0, "suspend": 1},
    {"rule": WOLFF, "field_cache": 1}, {"ones": 1, "row_shared_fields": 2, "n": 10000, "ldj": 10016, "sstride": 10240, "R": 1024},
    {"j_abs_max": 256, "row_shared_grid": 1, "grid_planes": 1}, {"consistent_dE": 0, "n_models": 3},
]


def line(traits):
    return " ".join(f"{k}={v}" for k, v in traits.items())


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """traits -> (what the parent commit could answer, the shared admission question), through the driver linked to libsga.so"""
    exe = str(tmp_path_factory.mktemp("window_forms") / "window_forms")
    subprocess.run([HIPCC] + HOST + [os.path.join(ROOT, "tests", "c_abi", "window_forms.cpp"), "-o", exe, "-L", CSRC, "-lsga",
                    "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out

    def ask(traits):
        return tuple(run([line(traits)])[0].split(" | "))
    ask.run = run
    return ask


def golden_table():
    with open(os.path.join(GOLDEN, "window_forms.json")) as f:
        return json.load(f)


# ----------------------------------------------------------------------------- against the parent commit
def test_the_table_is_the_grid():
    table = golden_table()
    assert "sga_impl::row_shared_window" in table["note"] and re.search(r"commit [0-9a-f]{7}", table["note"])
    assert table["bases"] == bases() and len(table["bases"]) == 18
    assert [(r["base"], r["flip"]) for r in table["rows"]] == [(b, f) for b in bases() for f in FLIPS]
    answers = {r["parent"] for r in table["rows"]}
    assert len(answers) > 60  # (the grid moves the answers: it is no table of one line)


def test_every_row_of_the_parent_commit_is_reproduced(forms):
    table = golden_table()
    lines = [line({**table["bases"][r["base"]], **r["flip"]}) for r in table["rows"]]
    for r, got in zip(table["rows"], forms.run(lines)):
        assert got.split(" | ")[0] == r["parent"], (r["base"], r["flip"])


# ----------------------------------------------------------------------------- by hand at the thresholds
def parse(answer):
    m = re.fullmatch(r"form=(-?\d+),(\d+) rs_w=(\d+) seq=(\d+),(\d+),(\d+) tiles=(\d+),(\d+),(.*)", answer[0])
    planes, grid, rs_w, sw, sgrid, mode, S, ones = (int(v) for v in m.groups()[:8])
    return dict(planes=planes, grid=grid, rs_w=rs_w, seq=(sw, sgrid, mode), tiles=(S, ones, m.group(9)), admit=answer[1])


def test_planes_by_the_largest_coupling(forms):
    for j, planes in ((1, 1), (2, 3), (7, 3), (8, 8), (255, 8), (256, 0)):
        a = parse(forms(dict(COMMON, j_abs_max=j)))
        assert a["planes"] == planes and a["grid"] == 0 and a["rs_w"] == (1024 if planes else 0), j
        assert a["admit"] == f"admit={planes},0,{j}"  # (the class exists at 256 too: the sequential form takes it)
        assert a["seq"] == (512, 0, 0 if j <= 127 else 1)
    for planes, jmax in ((1, 7), (3, 7), (8, 255)):
        a = parse(forms(dict(COMMON, table_m=0, row_shared_grid=1, grid_planes=planes, grid_k=2)))
        assert (a["planes"], a["grid"], a["rs_w"], a["admit"]) == (planes, 3, 1024, f"admit={planes},3,{jmax}")


def test_sequential_product_mode(forms):
    for i8 in (0, 1):
        for j, mode in ((127, 0), (128, 1)):
            assert parse(forms(dict(COMMON, want_i8=i8, j_abs_max=j)))["seq"] == (512, 0, 0 if i8 else mode)
    # the grid: 3 planes bound |2^k J| by 7 (int8 cores), 8 planes by 255 (fp32 cores)
    for planes, mode in ((1, 0), (3, 0), (8, 1)):
        assert parse(forms(dict(COMMON, table_m=0, row_shared_grid=1, grid_planes=planes, grid_k=1)))["seq"] == (512, 2, mode)
    # int8 rows are integers: k = 0 is taken, k >= 1 refused -- by the sequential form alone
    g = dict(COMMON, want_i8=1, table_m=0, row_shared_grid=1, grid_planes=3)
    a0, a1 = parse(forms(dict(g, grid_k=0))), parse(forms(dict(g, grid_k=1)))
    assert a0["seq"] == (512, 1, 0) and a1["seq"] == (0, 0, 0) and a0["rs_w"] == a1["rs_w"] == 1024


def test_replica_bounds(forms):
    big = dict(COMMON, n=2048, ldj=2048, sstride=2048)
    below, at = parse(forms(dict(big, R=(1 << 20) - 1))), parse(forms(dict(big, R=1 << 20)))
    assert (1 << 20) * 2048 == 1 << 31 and below["rs_w"] == 1024 and below["seq"][0] == 512  # R n = 2^31 - 2048
    assert at["rs_w"] == 0 and at["seq"][0] == 0 and at["admit"] == "admit=no(R n beyond 2^31 - 1)"
    # R n = 2^31 - 1 exactly (a prime): one replica of 2^31 - 1 spins for the row-shared form, 2^31 - 1 replicas of one spin for
    # the sequential form, which has no bound on R alone (the tiles, whose sizes are ints of n, are switched off)
    a = parse(forms(dict(COMMON, n=2 ** 31 - 1, R=1, ldj=2 ** 31, sstride=2 ** 31 - 16, row_shared_fields=0)))
    assert a["rs_w"] == 1024 and a["admit"] == "admit=1,0,1"
    a = parse(forms(dict(COMMON, n=1, R=2 ** 31 - 1, ldj=32, sstride=32, row_shared_fields=0)))
    assert a["seq"] == (512, 0, 0) and a["rs_w"] == 0 and a["admit"] == "admit=1,0,1"
    # ... and 2^31 with R below 2^20
    two = dict(COMMON, n=65536, ldj=65536, sstride=65536)
    assert parse(forms(dict(two, R=32767)))["rs_w"] == 1024 and parse(forms(dict(two, R=32767)))["seq"][0] == 512
    a = parse(forms(dict(two, R=32768)))
    assert a["rs_w"] == 0 and a["seq"][0] == 0 and a["admit"].startswith("admit=no(R n")
    # R alone: 2^20 replicas are refused by the row-shared form only
    small = dict(COMMON, n=100, ldj=128, sstride=128)
    assert parse(forms(dict(small, R=(1 << 20) - 1)))["rs_w"] == 1024
    a = parse(forms(dict(small, R=1 << 20)))
    assert a["rs_w"] == 0 and a["seq"] == (512, 0, 0) and a["admit"] == "admit=1,0,1"


def test_window_choice(forms):
    for fw, W in ((0, 1024), (255, 1024), (256, 256), (511, 256), (512, 512), (1023, 512), (1024, 1024)):
        assert parse(forms(dict(COMMON, row_shared_window=fw)))["rs_w"] == W, fw
        # a tuned pick fills in only where the option names no window
        assert parse(forms(dict(COMMON, row_shared_window=fw, tuned_w=512)))["rs_w"] == (512 if fw < 256 else W), fw
    two = dict(COMMON, row_shared=2, rule=GLAUBER, tuned_w=256)
    assert parse(forms(dict(two, tuned_rule=GLAUBER)))["rs_w"] == 256
    assert parse(forms(dict(two, tuned_rule=METROPOLIS)))["rs_w"] == 0
    assert parse(forms(dict(COMMON, row_shared=2)))["rs_w"] == 0
    # option 1 under a rule the pick was not timed for: the default window, not the pick
    assert parse(forms(dict(COMMON, rule=GLAUBER, tuned_w=256, tuned_rule=METROPOLIS)))["rs_w"] == 1024


def test_what_gates_one_form_only(forms):
    for flip in ({"suspend": 1}, {"row_shared": 0}, {"look_ahead": 0}, {"lean": 0}):
        a = parse(forms(dict(COMMON, **flip)))
        assert a["rs_w"] == 0 and a["seq"] == (512, 0, 0) and a["admit"] == "admit=1,0,1", flip
    for flip in ({"seq_w": 0}, {"sstride": 1000}, {"sstride": 992}, {"ldj": 992}):  # not a multiple of 16; below kpad = 1024
        a = parse(forms(dict(COMMON, **flip)))
        assert a["rs_w"] == 1024 and a["seq"] == (0, 0, 0), flip
    assert parse(forms(dict(COMMON, sstride=1000, R=0)))["seq"] == (512, 0, 0)  # (no replicas yet: no spin stride to hold)


def test_what_refuses_both(forms):
    for flip, why in (({"rule": WOLFF}, "the Wolff rule"), ({"field_cache": 1}, "cached local fields asked for"),
                      ({"field_cache": 2}, "cached local fields asked for"), ({"dense": 0}, "not a dense problem"),
                      ({"implicit": 1}, "not a dense problem"), ({"ragged": 1}, "not a dense problem"),
                      ({"n_models": 2}, "a stacked batch: one matrix per model"), ({"consistent_dE": 0}, "J not symmetric with a zero diagonal"),
                      ({"force_general": 1}, "option force_general"), ({"packed": 0}, "no couplings set"),
                      ({"acc64": 1}, "neither the integer class nor (option row_shared_grid = 1) a grid verdict"),
                      ({"table_m": 0}, "neither the integer class nor (option row_shared_grid = 1) a grid verdict")):
        a = parse(forms(dict(COMMON, **flip)))
        assert a["rs_w"] == 0 and a["seq"] == (0, 0, 0) and a["admit"] == f"admit=no({why})", flip
    for rule in (GLAUBER, HEAT_BATH):
        assert parse(forms(dict(COMMON, rule=rule)))["rs_w"] == 1024
    assert parse(forms(dict(COMMON, n_models=2, shared_j=1)))["admit"] == "admit=1,0,1"


# ----------------------------------------------------------------------------- sga_explain_route asks the same function
def test_explain_route_agrees_over_the_dense_cases(forms):
    import spin_glass_anneal_rl_amd as sg
    N = sg._native
    with open(os.path.join(GOLDEN, "route_table.json")) as f:
        dense = [c for c in json.load(f)["cases"] if c["query"]["kind"] == N.ROUTE_DENSE]
    assert len(dense) >= 10
    queries, seen = [], set()
    for c in dense:
        opts = dict(c["query"].get("options") or {})
        for extra, fields in (({"row_shared": 1}, {}), ({"row_shared": 1, "row_shared_grid": 1}, {}),
                              ({"row_shared": 1, "row_shared_grid": 1}, {"rs_grid": 3}), ({"row_shared": 1, "row_shared_window": 512}, {})):
            queries.append(N.route_query(**{**c["query"], **fields, "options": {**opts, **extra}}))
    out = forms.run(["query " + bytes(q).hex() for q in queries])
    for q, got in zip(queries, out):
        w, grid = (int(v) for v in re.fullmatch(r"rs_w=(\d+) grid=(\d+)", got).groups())
        want = "" if not w else f" sweep=row-shared(W={w}" + (f" grid=2^-{grid - 1})" if grid else ")")
        text = N.explain_route(q)
        part = re.search(r" sweep=row-shared\([^)]*\)", text)
        assert (part.group(0) if part else "") == want, text
        seen.add(want)
    assert seen == {"", " sweep=row-shared(W=1024)", " sweep=row-shared(W=1024 grid=2^-2)"}


# ----------------------------------------------------------------------------- sanitizers, stand-alone
def test_the_pure_half_under_the_sanitizers(tmp_path):
    """window_forms.cpp and sga_windows.cpp (its pure half alone: SGA_WINDOWS_PURE) as one program with its own main, built
    with the address and undefined-behaviour sanitizers, over the whole table: the same answers, no report."""
    exe = str(tmp_path / "window_forms_san")
    san = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run([HIPCC] + HOST + san + ["-DSGA_WINDOWS_PURE", os.path.join(ROOT, "tests", "c_abi", "window_forms.cpp"),
                                           os.path.join(CSRC, "sga_windows.cpp"), "-o", exe], check=True, capture_output=True)
    table = golden_table()
    lines = [line({**table["bases"][r["base"]], **r["flip"]}) for r in table["rows"]]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    assert [ln.split(" | ")[0] for ln in run.stdout.splitlines()] == [r["parent"] for r in table["rows"]]


# ----------------------------------------------------------------------------- the three resets of the forms' state
def test_what_each_reset_drops(tmp_path):
    """tests/c_abi/window_state.cpp fills WindowState with sentinels (no device memory) and prints, for each of the three
    resets, the members back at their defaults and the buffers handed to the release function."""
    exe = str(tmp_path / "window_state")
    subprocess.run([HIPCC] + HOST + [os.path.join(ROOT, "tests", "c_abi", "window_state.cpp"), "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    plan = "rs.cnt rs.off rs.tot rs.ent rs.base rs.bits rs.jp rs.jabs rs.W rs.log_w rs.nw32 rs.planes rs.log_rg rs.n_groups rs_R rs_n rs_grid"
    scratch = "rs.cnt rs.off rs.tot rs.ent rs.base rs.bits"
    assert out == [
        # a new W: the scratch of the window plan alone; the resident planes, the int8 copy and the tuned pick stay
        f"next_plan reset: {plan} | released: {scratch}",
        # new replicas: the sequential scratch and the autotuner's pick as well; what belongs to the problem stays
        f"next_replicas reset: tuned_w tuned_rule seq_base seq_base_w {plan} | released: {scratch} seq_base",
        # a new problem: its planes, int8 copy, flags and grid verdict, the pick; seq_base went with the replicas before
        f"next_problem reset: grid_planes grid_k jp jabs ones tiles_refused seq_j8 seq_j8_refused tuned_w tuned_rule {plan}"
        f" | released: {scratch} jp jabs seq_j8",
    ]
