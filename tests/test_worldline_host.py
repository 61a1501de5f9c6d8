"""World-line cluster updates (sga_worldline_clusters, csrc/worldline_clusters.hip), what holds without a GPU: the version,
the symbol in the library, the header and the binding; the reference of tests/worldline_reference.py -- its segments on
hand-written rings, its two limits against the oracle's single-spin rule, its tracked energies, and detailed balance of one
site update by exact enumeration; bond_probability, the p_bond shapes and the configuration checks; the admission rule run
stand-alone (tests/c_abi/worldline_plan.cpp).  tests/test_worldline_gpu.py holds the engine against the reference."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import oracle
import worldline_reference as wr
from test_transverse_host import small_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc")
SEED = (0x9E37 << 32) | 0x79B9  # above 2^32: both key words count


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


# ---- binding and reference basics ----------------------------------------------------------------------------------------
def test_version_symbol_header_binding(sg):
    assert sg._native.lib().sga_version() >= 3000
    assert hasattr(sg._native.lib(), "sga_worldline_clusters")
    assert "sga_worldline_clusters" in [s[0] for s in sg._native.SYMBOLS]
    header = open(os.path.join(ROOT, "include", "sga.h")).read()
    assert "int sga_worldline_clusters(sga_engine *e, int n_sweeps, int n_slices, uint32_t round," in header
    assert "bond_probability" in sg.__all__ and hasattr(sg, "bond_probability")
    assert hasattr(sg.AnnealEngine, "worldline_clusters")
    assert wr.DOMAIN_WORLDLINE == 4


def test_segments_on_hand_written_rings():
    up4 = [1, 1, 1, 1]
    # no head: every bond active -> the whole ring, head 0
    assert wr.segments(up4, [1, 1, 1, 1]) == [(0, [0, 1, 2, 3])]
    # one head: the one open bond 1 -> 2 makes slice 2 the head, the segment wraps through slice 0
    assert wr.segments(up4, [1, 0, 1, 1]) == [(2, [2, 3, 0, 1])]
    # the wrap through slice 0: bonds 3 -> 0 and 0 -> 1 active, the others open
    assert wr.segments(up4, [1, 0, 0, 1]) == [(2, [2]), (3, [3, 0, 1])]
    # no bond: every slice its own segment
    assert wr.segments(up4, [0, 0, 0, 0]) == [(0, [0]), (1, [1]), (2, [2]), (3, [3])]
    # a drawn bond between unequal spins is not active
    assert wr.segments([1, -1, -1, 1], [1, 1, 1, 1]) == [(1, [1, 2]), (3, [3, 0])]
    assert wr.segments([1, -1, 1, -1, 1], [1, 1, 1, 1, 1]) == [(1, [1]), (2, [2]), (3, [3]), (4, [4, 0])]
    # an odd ring
    assert wr.segments([1, 1, 1], [0, 1, 1]) == [(1, [1, 2, 0])]
    # P = 2: both bonds join the same pair; one is enough to join it, the head is the slice behind the open one
    assert wr.segments([1, 1], [1, 1]) == [(0, [0, 1])]
    assert wr.segments([1, 1], [1, 0]) == [(0, [0, 1])]
    assert wr.segments([1, 1], [0, 1]) == [(1, [1, 0])]
    assert wr.segments([1, 1], [0, 0]) == [(0, [0]), (1, [1])]
    assert wr.segments([1, -1], [1, 1]) == [(0, [0]), (1, [1])]
    assert wr.threshold(1.0) == 1 << 24 and wr.threshold(0.0) == 0 and wr.threshold(0.5) == 1 << 23
    assert wr.threshold(1.0 - 2.0 ** -25) == (1 << 24) - 1


# ---- the limits of the reference -----------------------------------------------------------------------------------------
def test_no_bonds_is_the_single_spin_rule():
    """thr = 0: every slice is its own segment, and its decision and dE are the oracle's Metropolis update of that slice at
    that site under the slice's own uniform, bit for bit."""
    rng = np.random.RandomState(11)
    n, P, T = 19, 3, 1.7
    prob = small_graph(n, rng, half_integer_h=True)
    S = oracle.init_spins(n, P, SEED)
    flips = stays = 0
    for rnd in range(2):
        for i in range(n):
            d = [wr.draws(SEED, i, rnd, 6 + p) for p in range(P)]
            before = S.copy()
            records, moved = wr.site_update(prob, S, i, T, 0, [x[0] for x in d], [x[1] for x in d])
            assert [(r["head"], r["members"]) for r in records] == [(p, [p]) for p in range(P)]
            for p in range(P):
                s = before[p].copy()
                took, dE = oracle.metropolis_update(prob, s, i, T, float(d[p][1]), arith=oracle.ARITH_F64)
                assert took == records[p]["flip"] and np.array_equal(s, S[p])
                assert moved[p] == dE  # (0.0 where the slice stays)
                s = before[p].copy()
                assert records[p]["dE"] == oracle.metropolis_update(prob, s, i, np.inf, 0.0, arith=oracle.ARITH_F64)[1]
                flips += took
                stays += not took
    assert flips > 10 and stays > 10


def test_all_bonds_on_identical_slices_is_one_replica_at_T_over_P():
    """thr = 2^24 and identical slices, P = 4, T = 2: the slices stay identical, and the walk is the one-replica typewriter
    Metropolis walk at T / P = 0.5 under slice 0's uniforms (powers of two keep -P dE / T exact)."""
    rng = np.random.RandomState(12)
    n, P, T = 21, 4, 2.0
    prob = small_graph(n, rng, half_integer_h=True)
    one = oracle.init_spins(n, 1, SEED)[0]
    S = np.repeat(one[None, :], P, axis=0).copy()
    out = wr.sweeps(prob, S, T, 3, P, 1.0, seed=SEED, round=5, replica0=8)
    E, flips = oracle.energy(prob, one), 0
    for kk in range(3):
        for i in range(n):
            took, dE = oracle.metropolis_update(prob, one, i, T / P, float(wr.draws(SEED, i, 5 + kk, 8)[1]))
            E += dE
            flips += took
    assert all(np.array_equal(S[p], one) for p in range(P))
    assert np.array_equal(out["energy"], np.full(P, E))
    assert np.array_equal(out["stats"], [[3 * n, flips, P * flips]]) and 0 < flips < 3 * n


@pytest.mark.parametrize("P,G", [(2, 2), (3, 1), (5, 2)])
def test_tracked_energies_are_classical(P, G):
    rng = np.random.RandomState(13 + P)
    n = 23
    prob = small_graph(n, rng, half_integer_h=True)
    S = oracle.init_spins(n, P * G, SEED)
    T = np.repeat(0.8 + 1.1 * np.arange(G), P)
    pb = rng.uniform(0.2, 0.9, (3, G))
    start = S.copy()
    out = wr.sweeps(prob, S, T, 3, P, pb, seed=SEED, round=2)
    assert np.array_equal(out["energy"], [oracle.energy(prob, s) for s in S])
    assert np.all(out["best_energy"] <= out["energy"]) and not np.array_equal(S, start)
    assert np.array_equal(out["best_energy"], [oracle.energy(prob, s) for s in out["best_spins"]])
    st = out["stats"]
    assert np.all(st[:, 0] >= st[:, 1]) and np.all(st[:, 2] >= st[:, 1]) and np.all(st[:, 1] > 0)
    assert np.all(st[:, 0] < 3 * n * P)  # some bonds were active
    # a call of 2 sweeps is a call of 1 at `round` and a call of 1 at `round + 1`; sharding by whole groups changes nothing
    a, b = start.copy(), start.copy()
    two = wr.sweeps(prob, a, T, 2, P, pb[:2], seed=SEED, round=2)
    first = wr.sweeps(prob, b, T, 1, P, pb[:1], seed=SEED, round=2)
    second = wr.sweeps(prob, b, T, 1, P, pb[1:2], seed=SEED, round=3, energy=first["energy"], best_energy=first["best_energy"],
                       best_spins=first["best_spins"])
    assert np.array_equal(a, b) and all(np.array_equal(two[key], second[key]) for key in ("energy", "best_energy", "best_spins"))
    assert np.array_equal(two["stats"], first["stats"] + second["stats"])
    if G > 1:
        part = start[P:].copy()
        wr.sweeps(prob, part, T[P:], 2, P, pb[:2, 1:], seed=SEED, round=2, replica0=P)
        assert np.array_equal(part, a[P:])


# ---- detailed balance by exact enumeration ------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 4, 6])
def test_detailed_balance_by_enumeration(sg, P):
    """One site update against pi ~ exp((k sum_p s_p s_{p+1} + sum_p s_p phi_p) / T) with p_bond = bond_probability(k, T):
    all 2^P columns x 2^P bond draws through the reference's segments, every segment flipping with min(1, exp(-dE / T)) in
    float64.  Rows sum to 1, and |pi_a M_ab - pi_b M_ba| <= 1e-12 of the largest flow: sums of <= 4096 terms in float64
    (observed 5e-17)."""
    rng = np.random.RandomState(P)
    k, T = 0.7, 1.3
    phi = rng.randint(-5, 6, P) / 2.0  # half-integer fields: phi_p stands for dot_p + h
    pb = sg.bond_probability(k, T)
    cols = list(itertools.product((1, -1), repeat=P))
    index = {c: a for a, c in enumerate(cols)}
    M = np.zeros((len(cols), len(cols)))
    for a, col in enumerate(cols):
        for draw in itertools.product((0, 1), repeat=P):
            w = float(np.prod([pb if d else 1.0 - pb for d in draw]))
            segs = wr.segments(list(col), list(draw))
            pf = []
            for f, members in segs:
                dE = 2.0 * col[f] * sum(phi[p] for p in members)
                pf.append(min(1.0, math.exp(-dE / T)))
            for choice in itertools.product((0, 1), repeat=len(segs)):
                new, pr = list(col), w
                for (f, members), flip, q in zip(segs, choice, pf):
                    pr *= q if flip else 1.0 - q
                    if flip:
                        for p in members:
                            new[p] = -col[p]
                if pr:
                    M[a, index[tuple(new)]] += pr
    logw = np.asarray([(k * sum(c[p] * c[(p + 1) % P] for p in range(P)) + float(np.dot(c, phi))) / T for c in cols])
    pi = np.exp(logw - logw.max())
    pi /= pi.sum()
    assert np.all(np.abs(M.sum(axis=1) - 1.0) <= 1e-12)
    flow = pi[:, None] * M
    assert np.max(np.abs(flow - flow.T)) <= 1e-12 * flow.max()
    # the chain moves: no column stays with certainty, and the whole ring flips as one with a probability of its own
    assert np.all(np.diag(M) < 1.0) and M[index[(1,) * P], index[(-1,) * P]] > 0.0


# ---- Python checks -----------------------------------------------------------------------------------------------------------
def test_bond_probability(sg):
    f = sg.bond_probability
    assert f(0.0, 1.0) == 0.0 and f(np.inf, 1.0) == 1.0 and isinstance(f(0.5, 2.0), float)
    k = np.asarray([1e-12, 0.01, 0.5, 3.0, 50.0])
    assert np.array_equal(f(k, 3.2), -np.expm1(-2.0 * k / 3.2)) and f(k, 3.2).dtype == np.float64
    assert f(1e-12, 1.0) == pytest.approx(2e-12, rel=1e-9)  # expm1, not 1 - exp
    assert np.all(np.diff(f(k, 3.2)) > 0) and np.all((f(k, 3.2) >= 0) & (f(k, 3.2) <= 1))
    assert f is sg.quantum.bond_probability
    for bad in ((-0.1, 1.0), ([0.5, -1e-9], 1.0), (float("nan"), 1.0), (0.5, 0.0), (0.5, -1.0), (0.5, float("inf")), (0.5, float("nan"))):
        with pytest.raises(sg.ConfigurationError):
            f(*bad)


def test_p_bond_shapes(sg):
    from spin_glass_anneal_rl_amd.engine import worldline_p_bond as f
    assert np.array_equal(f(0.5, 2, 3), np.full((2, 3), 0.5))
    assert np.array_equal(f([0.25, 1.0], 2, 3), [[0.25] * 3, [1.0] * 3])
    b = np.arange(6, dtype=np.float32).reshape(2, 3) / 8
    out = f(b, 2, 3)
    assert out.dtype == np.float64 and out.flags.c_contiguous and np.array_equal(out, b)
    assert f(1.0, 0, 3).shape == (0, 3)
    for bad in (np.zeros(3), np.zeros((3, 2)), np.zeros((2, 3, 1)), np.zeros((2, 2))):
        with pytest.raises(sg.AnnealingError):
            f(bad, 2, 3)


def test_config_checks(sg):
    C = sg.SimulatedQuantumAnnealingConfig
    assert C().worldline_clusters is False and C().cluster_interval == 1
    ok = C(n_slices=8, n_sweeps=10, worldline_clusters=True, cluster_interval=3)
    assert ok.worldline_clusters and ok.cluster_interval == 3
    for bad in (dict(cluster_interval=0), dict(cluster_interval=-1), dict(cluster_interval=1.5), dict(cluster_interval=True),
                dict(worldline_clusters=1), dict(worldline_clusters="yes"), dict(worldline_clusters=True, n_slices=66)):
        with pytest.raises(sg.ConfigurationError):
            C(**bad)
    assert C(n_slices=66).n_slices == 66  # the transverse sweeps alone serve it
    q = sg.QuantumFluctuations(None, "linear_decrease", 5.0, worldline_clusters=True)
    assert q.worldline_clusters is True and sg.QuantumFluctuations(None).worldline_clusters is False
    assert sg.SimulatedQuantumAnnealing(ok).cluster_statistics is None


# ---- the admission rule, stand-alone -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("worldline_plan")), "worldline_plan")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-I", "/opt/rocm/include",
                    os.path.join(ROOT, "tests", "c_abi", "worldline_plan.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def plan(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.strip()


ACC_TABLE, ACC_F32, ACC_F64, ACC_CANON = 0, 1, 2, 3
SERVED = dict(have_engine=1, have_p=1, n=100, R_local=12, replica0=0, sstride=112, csr=1, tsp=0, groups=0, ragged=0, n_models=1,
              csr_acc=ACC_TABLE, metropolis=1, consistent_dE=1, n_sweeps=3, n_slices=4)


def check(exe, p=(0.25,), **change):
    q = dict(SERVED, **change)
    return plan(exe, "check", *[q[key] for key in SERVED], *p)


def test_admission_rule(plan_exe):
    budget = 160 * 1024 - 256
    lines = plan(plan_exe, "sites", 2, 32, 33, 64).splitlines()
    assert lines[0] == "budget=%d" % budget
    rows = [[int(x) for x in line.split()] for line in lines[1:]]
    # the admitted n is computed from the transverse sweep's budget: one word per site, 64 int32 accumulators behind them
    assert [r[0] for r in rows] == [4, 4, 8, 8]
    assert rows[0][1] == rows[1][1] == (budget - 256) // 4 // 4 * 4 and rows[2][1] == rows[3][1] == (budget - 256) // 8 // 4 * 4
    assert all(r[2] <= budget for r in rows) and rows[0][1] > 40000 and rows[2][1] > 20000
    assert 22 ** 3 <= rows[0][1] and 10 ** 4 <= rows[2][1]  # both measured shapes fit
    # the thresholds: floor(p 2^24) in double
    assert plan(plan_exe, "thr", 0, 1, 0.5, 1.0 - 2.0 ** -25, 2.0 ** -24, 2.0 ** -25, 0.3).split() == \
        [str(x) for x in (0, 1 << 24, 1 << 23, (1 << 24) - 1, 1, 0, int(math.floor(0.3 * 2 ** 24)))]
    # served: both classes, every P in 2 ... 64 that divides R_local, odd ones included, any rule, p at both ends
    assert check(plan_exe) == "ok"
    assert check(plan_exe, csr_acc=ACC_F32) == "ok"
    for P in (2, 3, 4, 6, 12):
        assert check(plan_exe, n_slices=P) == "ok"
    for P in (32, 33, 34, 63, 64):
        assert check(plan_exe, n_slices=P, R_local=2 * P) == "ok"
    assert check(plan_exe, metropolis=0) == "ok"  # the call brings its own rule
    assert check(plan_exe, replica0=8) == "ok" and check(plan_exe, replica0=4, R_local=4) == "ok"
    assert check(plan_exe, p=(0.0, 1.0, 0.5, 1e-300)) == "ok"
    assert check(plan_exe, n_sweeps=0, p=("nan",)) == "ok"  # nothing of p_bond is read: the call is a no-op
    assert check(plan_exe, n=rows[0][1], sstride=rows[0][1]) == "ok"
    assert check(plan_exe, n=rows[2][1], sstride=rows[2][1], n_slices=64, R_local=64) == "ok"
    # invalid
    invalid = [dict(have_engine=0), dict(have_p=0), dict(n=0), dict(R_local=0), dict(n_sweeps=-1), dict(n_slices=1), dict(n_slices=0),
               dict(n_slices=-2), dict(n_slices=5), dict(n_slices=8), dict(n_slices=24), dict(n_slices=65, R_local=130),
               dict(n_slices=128, R_local=128), dict(replica0=2), dict(replica0=6)]
    for change in invalid:
        assert check(plan_exe, **change).startswith("invalid: "), change
    for p in (("nan",), ("inf",), (-1e-9,), (1.0000001,), (-0.5,), (0.5,) * 8 + ("nan",)):  # (the ninth and last of 3 x 3 values)
        assert check(plan_exe, p=p) == "invalid: p_bond holds a NaN or a value outside [0, 1]", p
    # an argument error is reported whatever the problem
    assert check(plan_exe, csr=0, n_slices=5).startswith("invalid: ")
    # unsupported, each with its reason
    unsupported = {"tsp": dict(tsp=1, csr=0), "groups": dict(groups=1, csr=0), "ragged": dict(ragged=1, n_models=3),
                   "batches": dict(n_models=3), "dense": dict(csr=0), "exact fp32": dict(csr_acc=ACC_F64), "canonical": dict(csr_acc=ACC_CANON),
                   "symmetric": dict(consistent_dE=0), "int8 spins do not fit LDS": dict(sstride=163600),
                   "spin words do not fit LDS": dict(n=rows[0][1] + 1, sstride=rows[0][1] + 16)}
    for word, change in unsupported.items():
        out = check(plan_exe, **change)
        assert out.startswith("unsupported: ") and word in out, (change, out)
    out = check(plan_exe, n=rows[2][1] + 1, sstride=rows[2][1] + 16, n_slices=33, R_local=33)
    assert out.startswith("unsupported: ") and "spin words" in out
    assert check(plan_exe, n=rows[2][1] + 1, sstride=rows[2][1] + 16, n_slices=32, R_local=32) == "ok"  # the 4-byte words still fit
