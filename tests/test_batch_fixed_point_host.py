"""Fixed-point cached local fields for many-model dense batches (option "batch_fixed_point"), what holds without a GPU:
the option and the version, the set-time classification (tests/c_abi/batch_fx_classify.cpp over sga_classify.cpp), the
route's answers for hand-filled queries, and the BatchConfig default."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import batch_fx_cases as cases
from conftest import ROOT

FX = "cached local fields (fixed point): "
EVERY = " (a dense batch: in every model)"
FX_BATCH = FX + "not built for dense batches (one model only)"
FX_CANON_BATCH = FX + ("the couplings need the canonical fp64 summation order (acc class f64-canonical: their binary places "
                       "span more than 53 bits over the stack, so no exact fixed point at one k holds a row sum; a dense "
                       "batch: in every model)")
FX_WIDE_BATCH = FX + "fields wider than int64 (a dense batch: in every model, at the batch-wide k)"


@pytest.fixture(scope="module")
def N():
    import spin_glass_anneal_rl_amd as sg
    return sg._native


def test_version_and_option(N):
    assert N.lib().sga_version() >= 1400
    names = N.option_names()
    assert "batch_fixed_point" in names
    # placed after every option but "ragged_field_cache", which stays last: the options before it keep their indices in
    # sga_route_query.opt[] (recorded queries name options by key)
    assert names[-2:] == ["batch_fixed_point", "ragged_field_cache"] and names.index("row_shared_window") == len(names) - 3
    q = N.RouteQuery()
    N.check(N.lib().sga_route_query_init(q))
    assert q.opt[names.index("batch_fixed_point")] == 0  # the default


def test_set_option_rejects_values_outside_zero_and_one():
    """sga_set_option needs an engine, and an engine a device: where there is none the range is read from the route's
    option table through the public header instead (the table sga_set_option checks against)."""
    import torch
    import spin_glass_anneal_rl_amd as sg
    if torch.cuda.is_available():
        with sg.AnnealEngine(0) as e:
            for bad in (-1, 2, 7):
                with pytest.raises(sg.AnnealingError):
                    e.set_option("batch_fixed_point", bad)
            for good in (1, 0):
                e.set_option("batch_fixed_point", good)
                assert e.get_option("batch_fixed_point") == good
    text = open(os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc", "sga_route.h")).read()
    assert '{"batch_fixed_point", "SGA_BATCH_FIXED_POINT", 0, 0, 0, 0, 1, 2},' in text  # default 0, range [0, 1], [set]


def _fx(name, bits=0, k=0, why="-"):
    return f"{name}: bits={bits} k={k} why={why}"


EXPECTED = {
    "cases": [
        _fx("case 0 clf=0 i8=0", 32, 10),   # A: binary grid 2^-10, sums of a few hundred
        _fx("case 1 clf=0 i8=0", 64, 10),   # B: 2^10 (2^24 + ...) >= 2^31, because of model 0
        _fx("case 2 clf=0 i8=1", 32, 0),    # C: integer J (k clamped at 0), quarter-valued h
        _fx("case 3 clf=0 i8=0", 32, 2),    # D: model 1's quarter-valued J sets the batch's k
        _fx("case 4 clf=0 i8=0", 32, 1),    # D's model 0 alone: k = 1
        _fx("case 5 clf=0 i8=0", 32, 10),   # B's model 1 alone: int32
        "asked=0"],
    "thresholds": [
        _fx("2047 k 20", 32, 20),           # 2047 2^20 (1 + 2^-20) < 2^31
        _fx("2048 k 20", 64, 20),
        _fx("k clamped", 32, 0)],
    "refusals": [
        _fx("all", why=FX_CANON_BATCH),
        "asked=0",
        _fx("diagonal", why=FX + "J must have a zero diagonal" + EVERY),
        _fx("asymmetric", why=FX + "J must be symmetric" + EVERY),
        _fx("width", why=FX_WIDE_BATCH),
        "asked=2",
        _fx("span", why=FX_CANON_BATCH)],
    "without the option": [
        _fx("three arguments, batch", why=FX_BATCH),
        _fx("batch_allowed = false, batch", why=FX_BATCH),
        _fx("three arguments, one model", 32, 20),
        _fx("batch_allowed = true, one model", 32, 20)],
}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_batch_verdicts_refusals_and_the_unchanged_three_argument_call(tmp_path):
    csrc = os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc")
    exe = str(tmp_path / "batch_fx_classify")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "c_abi", "batch_fx_classify.cpp"), "-o", exe, "-L", csrc, "-lsga",
                    "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    args = []
    Jd, hd = cases.case_d()
    Jb, hb = cases.case_b()
    for Js, hs in (cases.case_a(), (Jb, hb), cases.case_c(), (Jd, hd), (Jd[:1], hd[:1]), (Jb[1:], hb[1:])):
        args += [Js.shape[1], Js.shape[0]] + cases.scan_words(Js, hs)
    out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout
    got, name = {}, None
    for line in out.splitlines():
        if line.startswith("# "):
            name = line[2:]
            got[name] = []
        else:
            got[name].append(line)
    assert list(got) == list(EXPECTED)
    for name, lines in EXPECTED.items():
        assert got[name] == lines, (name, got[name])


# ----------------------------------------------------------------------------- the route, queries filled by hand
def _query(N, n=200, bits=32, option=1, R_local=12, cache=1):
    names = N.option_names()
    q = N.RouteQuery()
    N.check(N.lib().sga_route_query_init(q))
    q.kind, q.n, q.n_models, q.R_local = N.ROUTE_DENSE, n, 3, R_local
    q.storage, q.acc, q.clf_ok, q.clf_bits = N.J_F32, 1, 0, bits
    q.field_cache = cache
    q.ldj = (n + 31) // 32 * 32
    q.sstride = (n + 31) // 32 * 32
    q.opt[names.index("clf_fixed_point")] = 1
    q.opt[names.index("batch_fixed_point")] = option
    return q


def _cached(N, q):
    return N.explain_route(q).split(" cached=")[1]


@pytest.mark.parametrize("R_local", [0, 12])
@pytest.mark.parametrize("bits", [32, 64])
def test_route_names_the_batch_under_the_option(N, bits, R_local):
    on = _cached(N, _query(N, bits=bits, R_local=R_local, cache=1))
    assert on == f"on(waves=1 fields=int{bits} fixed-point models=3)", on
    auto = _cached(N, _query(N, bits=bits, R_local=R_local, cache=2))
    theta = (0.30 + 0.12 * 0.2) / (1.3 if bits == 32 else 1.5)  # the one-model dense fixed-point break-even
    assert auto == f"auto(start=rows theta={theta:.3f} models=3)", auto
    # the option at 0: the string such a query gave before the option existed (no "models=" in the ON answer)
    assert _cached(N, _query(N, bits=bits, R_local=R_local, option=0, cache=1)) == f"on(waves=1 fields=int{bits} fixed-point)"
    assert _cached(N, _query(N, bits=bits, R_local=R_local, option=0, cache=2)) == auto


def test_route_refusals(N):
    # int64 fields of 25 000 spins do not fit LDS -- asked only once replicas exist
    assert _cached(N, _query(N, n=25000, bits=64, R_local=12, cache=1)) == "refused"
    assert _cached(N, _query(N, n=25000, bits=64, R_local=12, cache=2)) == "unavailable"
    assert _cached(N, _query(N, n=25000, bits=64, R_local=0, cache=1)).startswith("on(")
    assert _cached(N, _query(N, n=25000, bits=32, R_local=12, cache=1)).startswith("on(")
    # the set-time scan refused the batch (clf_bits = 0): refused with and without the option
    for option in (0, 1):
        assert _cached(N, _query(N, bits=0, option=option, cache=1)) == "refused"
        assert _cached(N, _query(N, bits=0, option=option, cache=2)) == "unavailable"


def test_batch_config_default_and_validation():
    import spin_glass_anneal_rl_amd as sg
    assert sg.BatchConfig().stacked_fixed_point is False
    assert sg.BatchConfig(stacked_fixed_point=True).stacked_fixed_point is True
    with pytest.raises(ValueError):
        sg.BatchConfig(stacked_fixed_point="yes")


def test_scan_words_of_the_cases_are_what_the_verdicts_assume():
    """The words handed to the classifier above: A and B on the 2^-10 grid, C integer, D on the quarter grid."""
    for (Js, hs), lo_word, integer in ((cases.case_a(), 1034, False), (cases.case_b(), 1034, False),
                                       (cases.case_c(), 1024, True), (cases.case_d(), 1026, False)):
        w = cases.scan_words(Js, hs)
        assert w[6] == lo_word and (w[3] & 1) == (0 if integer else 1), w
    wb = cases.scan_words(*cases.case_b())
    assert wb[5] == 1024 + 24 and np.int32(wb[2]).view(np.float32) >= 2.0 ** 24
