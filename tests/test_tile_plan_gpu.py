"""The tile kernel's plan (csrc/sweep_dense_rs.hip, rs_tile_plan_kernel): the sweep's entries sorted by (window, slice of
rg replicas, tile, replica) in one launch, and rs_fields_tiles_kernel reading its tile's runs, one per slice.  None of it
may show in a result: with the harness of test_row_shared_tiles_gpu.py, the full state under "row_shared_fields" = 1
equals the per-site fields kernel's (which keeps the by-site plan), the row-per-proposal kernel's and, up to 130
replicas, the CPU oracle's, over a script of sweeps and exchanges (2, 1, 2).  The cases sit on the edges of the new
geometry: slices (rg asked of the host function), cut windows, chunks of the entry buffer that end inside a replica's run
and at a slice's end, tile ranges, empty tiles.

test_tile_ranges holds the smallest n whose tiles a workgroup covers in ranges at 3 replicas and tiles of 2 sites, and
its neighbour: counters for 20 192 tiles fit the plan's LDS, so n = 40 385 and 40 384 -- two dense problems of 6.5 GB
each, made on the device; the test takes about 25 s, most of it the oracle's and the copies'."""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tile_plan_rule as tp  # noqa: E402
from batch_fx_cases import oracle_batch  # noqa: E402
from oracle_engine import OracleEngine  # noqa: E402
from test_row_shared_tiles_gpu import (INF, assert_kernel, assert_same, check_case, couplings, engine_run, fields, ladder,  # noqa: E402
                                       run, select, state, temps_for)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    exe = tp.build(tmp_path_factory.mktemp("rs_tile_plan_rule"))

    def ask(n, W, S, R):
        rg, tiles, _, fit = tp.ask(exe, [(n, W, S, R)])[1][0]
        assert (rg, tiles) == tp.plan(n, W, S, R) and rg > 0 and fit == 1
        return rg, tiles
    return ask


# ----------------------------------------------------------------------------- slices
@pytest.mark.parametrize("S", [2, 64])
@pytest.mark.parametrize("which", ["rg-1", "rg", "rg+1", "2rg+1"])
def test_slice_edges(sg, rule, S, which):
    """A last slice of rg - 1 replicas, a full one, a slice of one replica behind one and behind two full ones."""
    n, W = 257, 256
    rg = rule(n, W, S, 33)[0]
    R = {"rg-1": rg - 1, "rg": rg, "rg+1": rg + 1, "2rg+1": 2 * rg + 1}[which]
    assert rule(n, W, S, R) == (rg, -(-n // S)) and rg == 32  # (one geometry for the four: the slices are what moves)
    check_case(sg, n, "pm1", R, W, "f32", S, ones=True)


@pytest.mark.parametrize("n", [300, 301])
def test_cut_last_window(sg, n):
    """W = 256: the second window has 44 updates per replica (whole Philox blocks) or 45 (half of the last block)."""
    check_case(sg, n, "pm1", 5, 256, "f32", 3, ones=True)


def test_chunk_boundaries(sg, rule):
    """n = 64 in one tile, 130 replicas: 8320 entries, two chunks of the entry buffer.  Slices of 32 replicas hold 2048
    entries each: the chunk ends at entry 6144, the end of the third slice, and the window's entries of a replica (64) do
    not divide the 6144 / 16 / 4 = 96 entries of a quarter wave's piece -- pieces end inside replicas' runs."""
    assert rule(64, 256, 64, 130) == (32, 1) and 3 * 32 * 64 == 6144
    check_case(sg, 64, "a7", 130, 256, "f32", 64, ones=False)
    # 6144 is no multiple of 50 entries per replica: the chunk ends inside the run of a replica, inside a slice
    check_case(sg, 50, "a7", 130, 256, "f32", 64, ones=False)


def test_one_replica(sg, rule):
    assert rule(257, 256, 2, 1)[0] == 32
    check_case(sg, 257, "pm1", 1, 256, "f32", 2, ones=True)
    check_case(sg, 1000, "tern", 1, 512, "i8", 0, ones=False)


def test_a_tile_without_an_entry_between_live_ones(sg):
    """n = 1000 at W = 256 with 3 replicas: 768 proposals per window over 500 tiles of two sites -- about a fifth of the
    tiles have no entry, most of the others one row nobody proposes."""
    check_case(sg, 1000, "a7", 3, 256, "f32", 2, ones=False)
    check_case(sg, 1000, "pm1", 3, 256, "f32", 2, ones=True)


@pytest.mark.parametrize("kind,ones", [("pm1", True), ("tern", False), ("a7", False), ("a100", False)])
def test_sign_only_and_general_planes(sg, kind, ones):
    """Sign-only rows and 1, 3 and 8 magnitude planes, two slices, the host rule's S."""
    check_case(sg, 257, kind, 33, 256, "f32", 0, ones=ones)


# ----------------------------------------------------------------------------- tile ranges
def device_couplings(n, seed):
    """+-1 couplings made on the device (symmetric, zero diagonal), and the same as a host array for the oracle."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.triu(torch.randint(0, 2, (n, n), generator=g, device="cuda", dtype=torch.int8) * 2 - 1, 1)
    J = (A + A.T).float()
    del A
    return J


def test_tile_ranges(sg, rule):
    """Both sides of the bound where a workgroup of the plan covers its tiles in ranges (see the module's docstring)."""
    R, W, S, script = 3, 256, 2, (2, 1, 2)
    n = 2
    while tp.plan(n, W, S, R)[1] >= -(-n // S):
        n += 1
    assert n == 40385
    assert rule(n, W, S, R) == (1, 20192) and rule(n - 1, W, S, R) == (1, 20192)  # 20 193 tiles: two ranges; 20 192: one
    for m in (n - 1, n):
        J = device_couplings(m, m)
        h = fields(m, "pm1", m)
        temps = temps_for(m, R, "pm1")
        got = {mode: engine_run(sg, J, h, R, W, "i8", mode, temps, 77, list(script), S if mode == "tiles" else 0, ones=True)
               for mode in ("tiles", "site", "rows")}
        assert_same(got["tiles"], got["site"], "per-site fields kernel")
        assert_same(got["tiles"], got["rows"], "row-per-proposal kernel")
        o = OracleEngine(J=J.cpu().numpy(), h=np.array(h))
        del J
        o.init_replicas(R, seed=77)
        o.set_ladder(temps)
        assert_same(got["tiles"], run(o, R, list(script)), "oracle")
        del o


# ----------------------------------------------------------------------------- shards, extremes, order, the autotuner
def test_shared_coupling_shard_with_replica0(sg):
    """sga_set_dense_shared, 4 field vectors x 10 replicas over one +-1 matrix, the second half of the replicas as a shard
    of its own (replica0 = 20: the plan's Philox coordinates are global, its slices local)."""
    n, M, k, W, seed, plan = 300, 4, 10, 256, 0x711E6, (2, 1, 2)
    R = M * k
    J = np.array(couplings(n, "pm1", 8))
    hs = np.stack([np.random.RandomState(60 + m).randint(-1, 2, n).astype(np.float32) for m in range(M)])
    temps = np.tile(ladder(k, 26.0, 2.6), M)
    ref = oracle_batch(np.ascontiguousarray(np.broadcast_to(J, (M,) + J.shape)), hs, k, seed, temps, plan, exchange=False)
    r0 = R // 2
    got = {}
    for mode in ("tiles", "site"):
        with sg.AnnealEngine(0) as e:
            select(e, mode, W, S=7 if mode == "tiles" else 0)
            e.set_dense_shared(J, hs, storage="f32")
            e.init_replicas(R - r0, seed=seed, R_global=R, replica0=r0)
            e.set_temperatures(temps[r0:])
            traces = []
            for ns in plan:
                traces.append(e.sweep(ns, energy_trace=True)["energy_trace"])
                assert_kernel(e, mode, 7 if mode == "tiles" else 0, ones=True if mode == "tiles" else None)
            got[mode] = dict(state(e, R - r0), trace=np.vstack(traces))
    assert_same(got["tiles"], got["site"], "per-site fields kernel")
    assert np.array_equal(got["tiles"]["trace"], np.concatenate(ref["traces"])[:, r0:])
    assert np.array_equal(got["tiles"]["spins"], ref["spins"][r0:]) and np.array_equal(got["tiles"]["accepted"], ref["acc"][r0:])
    assert np.array_equal(got["tiles"]["best_energy"], ref["best_e"][r0:]) and np.array_equal(got["tiles"]["best_spins"], ref["best_s"][r0:])


def test_zero_and_infinite_temperature_in_one_run(sg):
    """T = inf replicas accept every proposal, T = 0 ones only what does not raise the energy: both in the slices of one
    run, beside finite temperatures."""
    n, R, ns, seed = 300, 35, 4, 5
    J, h = couplings(n, "pm1", 8), fields(n, "pm1", n)
    sched = np.tile(np.resize(np.asarray([INF, 0.0, 10.0, 1.25, 0.0, INF, 3.0]), R), (ns, 1))
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(oracle.Problem(J=np.array(J), h=np.array(h)), s, sched, ns, seed=seed, n_threads=16)
    assert ref["n_accepted"][0] == ref["n_accepted"][5] == ns * n
    with sg.AnnealEngine(0) as e:
        select(e, "tiles", 256, S=7)
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        out = e.sweep(ns, sched=sched, energy_trace=True)
        assert_kernel(e, "tiles", 7, ones=True)
        assert np.array_equal(out["energy_trace"], ref["energy_trace"])
        assert np.array_equal(e.spins(), s) and np.array_equal(e.stats()[0], ref["n_accepted"])
        for r in range(R):
            be, bs, _ = e.best(r)
            assert be == ref["best_energy"][r] and np.array_equal(bs, ref["best_spins"][r])


def test_two_runs_leave_identical_state(sg):
    """The LDS atomics of the plan order a (tile, replica) bucket differently from run to run; every entry names its own
    base slot."""
    n, R, W = 1000, 200, 512
    J, h, temps = couplings(n, "pm1", 5), fields(n, "pm1", 6), ladder(R, 10.0, 0.1)
    a = engine_run(sg, J, h, R, W, "f32", "tiles", temps, 4243, [2, 1, 2], ones=True)
    b = engine_run(sg, J, h, R, W, "f32", "tiles", temps, 4243, [2, 1, 2], ones=True)
    assert_same(a, b, "second run")


def test_autotune_in_mid_run_leaves_no_trace(sg):
    """Default options at n = 7968, 8 replicas -- the default range of the tiles: sga_autotune times the three windows, each
    with the tile plan, on the live replicas, and the chain goes on as if it had not."""
    n, R, seed = 7968, 8, 99
    J, h, temps = couplings(n, "pm1", 41), fields(n, "pm1", n), temps_for(n, R, "pm1")
    s = oracle.init_spins(n, R, seed)
    ref = oracle.sweeps(oracle.Problem(J=np.array(J), h=np.array(h)), s, temps, 3, seed=seed, n_threads=8)
    with sg.AnnealEngine(0) as e:
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_ladder(temps)
        a = e.sweep(1, energy_trace=True)
        before = (e.spins(), e.energies(), e.best()[0], e.stats()[0], e.counters())
        e.autotune()
        after = (e.spins(), e.energies(), e.best()[0], e.stats()[0], e.counters())
        for x, y in zip(before, after):
            assert np.array_equal(np.asarray(x), np.asarray(y))
        forms = {key for key in e.autotune_table(forms=True) if key.startswith("row-shared:")}
        assert forms == {"row-shared:W256", "row-shared:W512", "row-shared:W1024"}, forms
        b = e.sweep(2, energy_trace=True)
        if "sweep=row-shared(W=" in e.describe():  # (which form wins is a measurement)
            assert " in tiles of " in e.last_kernel() and "sign-only" in e.last_kernel(), e.last_kernel()
        assert np.array_equal(np.concatenate([a["energy_trace"], b["energy_trace"]]), ref["energy_trace"])
        assert np.array_equal(e.spins(), s) and np.array_equal(e.stats()[0], ref["n_accepted"])
        for r in range(R):
            be, bs, _ = e.best(r)
            assert be == ref["best_energy"][r] and np.array_equal(bs, ref["best_spins"][r])
