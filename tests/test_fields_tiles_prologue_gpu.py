"""The tile kernel's prologue and entry loop (csrc/sweep_dense_rs.hip, rs_fields_tiles_kernel / rs_tile_pieces): the run
bounds read once, the row constants and plane rows loaded at kernel entry and dealt flat to the threads, the entries copied
flat with each one's run found by bisecting the prefix in LDS, and the entry loop's addresses as 32-bit byte offsets.  None
of it may show in a result: spins, energies, accept counters, best states and the energy trace over a script of sweeps with
exchange rounds in between under "row_shared_fields" = 1 equal -- not: are close to -- the per-site fields kernel
("row_shared_fields" = 0), the row-per-proposal kernel ("row_shared" = 0) and, for R <= 130, the CPU oracle.  Every case
asserts from last_kernel() / describe() that the tiles ran, so a silent fallback fails it.

The shapes are the smallest at which the new paths differ:
  * words of 16 bytes per lane and the partial last word: n = 300 (one word, lanes 0-3 of a quarter wave live), 2049 (two
    words, the last on two lanes), 4100 (three words; eight magnitude planes stream the bits instead);
  * tiles: S = 2 (fewer rows than waves; at one replica most tiles go unproposed: the early return), 24 (n % S != 0: a
    partial last tile), S = n and S > n (one tile: every entry of the window in one workgroup);
  * runs: one replica (one run), 33 (a slice of one replica behind a full one), 65 in two groups ([0, 64) and [64, 65)),
    130 (five slices of the largest size; more, and empty runs, where the plan takes smaller slices);
  * W = 256 and 1024; n = 300 at W = 256 has a cut second window of 44 updates;
  * chunks of the entry buffer: n = 300, W = 256, S = 96, 130 replicas put about 10 600 entries of the first window on a
    tile against a buffer of 6144 -- two chunks, the cut inside a replica's run;
  * instantiations: +-1 (sign-only), ternary with zeros (one general plane), |J| <= 7 (three), |J| <= 100 (eight).
Temperatures: replicas 0, 16, 32, ... run at T = inf and 1, 17, 33, ... at T = 0 (a lone replica: either), so every case
and every slice of 16 or 32 replicas holds both; the others sit on a geometric ladder."""
import functools
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_engine import OracleEngine  # noqa: E402
from test_row_shared_tiles_gpu import INF, assert_kernel, assert_same, couplings, fields, select, state, temps_for  # noqa: E402

pytestmark = pytest.mark.gpu

SCRIPT = (2, 1, 2)  # sweeps, an exchange round between the blocks
ENTRY_BUFFER = 6144  # RS_TILE_ENTRIES of sga_kernels.h


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def run(e, R, script, trace):
    """script: a list of sweep counts, an exchange round after each block but the last; trace: with the energy trace (which
    takes one replica group, so the cases in two groups run without)."""
    rows = []
    for i, ns in enumerate(script):
        out = e.sweep(ns, energy_trace=trace)
        if trace:
            rows.append(out["energy_trace"])
        if i + 1 < len(script):
            e.exchange()
    out = state(e, R)
    if trace:
        out["trace"] = np.vstack(rows)
    return out


def temps_of(n, R, kind, lone=INF):
    t = np.array(temps_for(n, R, kind))
    if R == 1:
        t[0] = lone
    else:
        t[0::16] = INF
        t[1::16] = 0.0
    return t


def problem(n, kind, R):
    return couplings(n, kind, 31 + n + R), fields(n, kind, n), 3000 + n + R


def engine_run(sg, n, kind, R, W, mode, temps, script, S=0, G=0, ones=None, trace=True):
    J, h, seed = problem(n, kind, R)
    with sg.AnnealEngine(0) as e:
        select(e, mode, W, S)
        if G:
            e.set_replica_groups(G)
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed)
        e.set_ladder(temps)
        out = run(e, R, script, trace)
        assert_kernel(e, mode, S if S <= n else 0, ones)
        if mode == "tiles":
            assert " in tiles of " in e.last_kernel(), e.last_kernel()
            if G > 1:
                assert e.last_kernel().endswith(f" groups={G}"), e.last_kernel()
    return out


@functools.lru_cache(maxsize=None)
def reference_runs(n, kind, R, W, lone, script, trace):
    """The per-site fields kernel, the row-per-proposal kernel and (R <= 130) the oracle on the case, once for every tile
    size and group count."""
    import spin_glass_anneal_rl_amd as sg
    temps = temps_of(n, R, kind, lone)
    refs = {mode: engine_run(sg, n, kind, R, W, mode, temps, script, trace=trace) for mode in ("site", "rows")}
    if R <= 130:
        J, h, seed = problem(n, kind, R)
        one_thread = oracle.sweeps
        oracle.sweeps = functools.partial(one_thread, n_threads=16)
        try:
            o = OracleEngine(J=np.array(J), h=np.array(h))
            o.init_replicas(R, seed=seed)
            o.set_ladder(temps)
            refs["oracle"] = run(o, R, script, trace)
        finally:
            oracle.sweeps = one_thread
    return refs


def check_case(sg, n, kind, R, W, S, G=0, lone=INF, script=SCRIPT):
    trace = G == 0
    new = engine_run(sg, n, kind, R, W, "tiles", temps_of(n, R, kind, lone), script, S, G, ones=(kind == "pm1"), trace=trace)
    refs = reference_runs(n, kind, R, W, lone, script, trace)
    assert set(refs) == ({"site", "rows", "oracle"} if R <= 130 else {"site", "rows"})
    for name, ref in refs.items():
        assert_same(new, ref, name)
    assert 0 < new["accepted"].sum() < sum(script) * n * R or R == 1
    return new


# ----------------------------------------------------------------------------- words per lane, instantiations
@pytest.mark.parametrize("kind", ["pm1", "tern", "a7", "a100"])
@pytest.mark.parametrize("n,W", [(300, 256), (2049, 1024), (4100, 1024)])
def test_word_counts_and_instantiations(sg, n, W, kind):
    check_case(sg, n, kind, 33, W, 24, script=SCRIPT if n < 4000 else (1, 1))


# ----------------------------------------------------------------------------- tile sizes against run structures
@pytest.mark.parametrize("R", [1, 33, 130])
@pytest.mark.parametrize("S", [2, 24, 300, 512])
def test_tile_sizes(sg, S, R):
    check_case(sg, 300, "pm1", R, 256, S)


@pytest.mark.parametrize("S", [2, 24])
def test_one_cold_replica(sg, S):
    """T = 0 on the lone replica (test_tile_sizes runs it at T = inf)."""
    check_case(sg, 300, "pm1", 1, 256, S, lone=0.0)


@pytest.mark.parametrize("kind,S,R", [("a7", 2, 1), ("a7", 24, 130), ("tern", 300, 33), ("a100", 24, 130)])
def test_tile_sizes_general_planes(sg, kind, S, R):
    check_case(sg, 300, kind, R, 256, S)


# ----------------------------------------------------------------------------- two groups, both windows
@pytest.mark.parametrize("kind", ["pm1", "tern"])
@pytest.mark.parametrize("n,W,S", [(300, 256, 24), (2049, 1024, 96)])
def test_two_groups_of_64_and_1(sg, n, W, S, kind):
    check_case(sg, n, kind, 65, W, S, G=2)


@pytest.mark.parametrize("kind", ["pm1", "a7"])
def test_window_of_1024_at_130_replicas(sg, kind):
    check_case(sg, 2049, kind, 130, 1024, 24)


# ----------------------------------------------------------------------------- chunks of the entry buffer
@pytest.mark.parametrize("kind", ["pm1", "a7"])
def test_two_chunks_cut_inside_a_run(sg, kind):
    n, W, S, R = 300, 256, 96, 130
    # the first window's entries on a tile: every replica proposes W sites, S / n of them in the tile on average (about 82
    # a replica, so the buffer ends inside the 75th replica's run or thereabouts)
    assert ENTRY_BUFFER < R * W * S // n < 2 * ENTRY_BUFFER
    check_case(sg, n, kind, R, W, S)
