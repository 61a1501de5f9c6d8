"""Isoenergetic cluster moves on the device (sga_cluster_move_pairs / sga_cluster_move_ladders, csrc/cluster_moves.hip).
The move is a deterministic function of the two configurations, the graph and one drawn integer, so every comparison is
np.array_equal against the breadth-first search of tests/cluster_reference.py: the flipped set, both replicas, every
other replica and site, the sizes, the accept counters, the energies (the oracle's, and what recompute_energies()
leaves), E_a + E_b, and the bests.  Couplings are integer +-1 unless a case says otherwise; spins come in through s0."""
import numpy as np
import pytest
import torch

import cluster_reference as cr
import groups_cases as gc
import oracle

pytestmark = pytest.mark.gpu

SEED = (0x9E37 << 32) | 0x79B9  # above 2^32: both key words count
ROUNDS = (0, 1, 2 ** 32 - 1)


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


# ---- graphs: (rowptr, colidx, val) with both triangles, rows sorted by column ------------------------------------------
def csr_from_edges(n, edges):
    rows = [dict() for _ in range(n)]
    for i, j, v in edges:
        assert i != j and j not in rows[i]
        rows[i][j] = v
        rows[j][i] = v
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.asarray([j for r in rows for j in sorted(r)], np.int32)
    val = np.asarray([r[j] for r in rows for j in sorted(r)], np.float32)
    return rowptr, col, val


def pm(rng):
    return float(rng.randint(0, 2) * 2 - 1)


def ring(n, rng):
    return csr_from_edges(n, [(i, (i + 1) % n, pm(rng)) for i in range(n)])


def path(n, rng, zero_bonds=()):
    return csr_from_edges(n, [(i, i + 1, 0.0 if i in zero_bonds else pm(rng)) for i in range(n - 1)])


def torus(Lx, rng):
    idx = lambda x, y: (x % Lx) * Lx + (y % Lx)  # noqa: E731
    return csr_from_edges(Lx * Lx, [(idx(x, y), idx(x + dx, y + dy), pm(rng)) for x in range(Lx) for y in range(Lx)
                                    for dx, dy in ((1, 0), (0, 1))])


def star(leaves, rng):
    return csr_from_edges(leaves + 1, [(0, j, pm(rng)) for j in range(1, leaves + 1)])


def random_graph(n, picks, rng):
    edges = {}
    for i in range(n):
        for j in rng.choice(n, picks, replace=False):
            if i != j:
                edges[(min(i, j), max(i, j))] = pm(rng)
    return csr_from_edges(n, [(i, j, v) for (i, j), v in sorted(edges.items())])


def random_spins(R, n, rng):
    return (rng.randint(0, 2, (R, n)) * 2 - 1).astype(np.int8)


def engine(sg, graph, h, s0, seed=SEED, cache=None, **replicas):
    e = sg.AnnealEngine(0)
    if cache is not None:
        e.set_field_cache(cache)
    e.set_csr(*graph, h)
    e.init_replicas(len(s0), seed=seed, s0=s0, **replicas)
    return e


def bests(e):
    out = [e.best(r) for r in range(e.R)]
    return np.asarray([b[0] for b in out]), np.stack([b[1] for b in out])


def state(e):
    be, bs = bests(e)
    return dict(S=e.spins(), E=e.energies(), acc=e.stats()[0], be=be, bs=bs)


def oracle_energies(graph, H, S, model_of=lambda r: 0):
    """The oracle's energy of every row; H [M, n]: row r lies under field vector model_of(r)."""
    H = np.atleast_2d(H)
    probs = [oracle.Problem(csr=graph, h=h) for h in H]
    return np.asarray([oracle.energy(probs[model_of(r)], S[r]) for r in range(len(S))])


def check_move(e, graph, H, pairs, rnd, seed, before, sizes, model_of=lambda r: 0):
    """The engine after one cluster call over `pairs` (local indices) against the reference applied to `before`."""
    want = before["S"].copy()
    want_sizes, want_acc = [], before["acc"].copy()
    for a, b in pairs:
        sa, sb, comp = cr.move(*graph, before["S"][a], before["S"][b], seed, rnd, e.replica0 + min(a, b))
        want[a], want[b] = sa, sb
        want_sizes.append(comp.size)
        want_acc[a] += comp.size
        want_acc[b] += comp.size
        # (the reference's own property: the component is flipped in both, so the pair's differing sites stay the same)
        assert np.array_equal(sa != sb, before["S"][a] != before["S"][b])
    now = state(e)
    assert np.array_equal(now["S"], want)  # the flipped set, in both replicas; every other replica and site unchanged
    assert np.array_equal(np.asarray(sizes).reshape(-1), want_sizes)
    assert np.array_equal(now["acc"], want_acc)
    # energies: the oracle's of the new rows; the untouched replicas' are the very numbers they were
    E_ref = oracle_energies(graph, H, want, model_of)
    assert np.array_equal(now["E"], E_ref)
    moved = np.any(want != before["S"], axis=1)
    assert np.array_equal(now["E"][~moved], before["E"][~moved])
    for a, b in pairs:
        assert now["E"][a] + now["E"][b] == before["E"][a] + before["E"][b]
    # bests: lowered only where the energy went down
    lower = now["E"] < before["be"]
    assert np.array_equal(now["be"], np.where(lower, now["E"], before["be"]))
    assert np.array_equal(now["bs"], np.where(lower[:, None], want, before["bs"]))
    e.recompute_energies()
    assert np.array_equal(e.energies(), now["E"])
    return now, want_sizes


def run_rounds(sg, graph, h, s0, pairs, rounds=ROUNDS, seed=SEED, **replicas):
    """One engine, one cluster call per round over `pairs`, each held against the reference.  Returns all sizes."""
    sizes_all = []
    with engine(sg, graph, h, s0, seed=seed, **replicas) as e:
        before = state(e)
        assert np.array_equal(before["E"], oracle_energies(graph, h, s0))
        for rnd in rounds:
            sizes = e.cluster_move_pairs(pairs, round=rnd)
            assert sizes.dtype == np.int32
            before, ws = check_move(e, graph, h, pairs, rnd, seed, before, sizes)
            sizes_all += ws
    return sizes_all


# ---- 1. the pair form against the reference --------------------------------------------------------------------------
def test_ring_arcs_and_many_levels(sg):
    n, rng = 300, np.random.RandomState(1)
    g = ring(n, rng)
    s0 = random_spins(4, n, rng)
    s0[1] = s0[0]
    for lo, hi in ((0, 150), (160, 201), (250, 261), (297, 300)):  # arcs of differing sites; the first takes 150 levels from its end
        s0[1, lo:hi] = -s0[0, lo:hi]
    h = rng.randint(-1, 2, n).astype(np.float32)  # a non-zero integer field: E_a + E_b is conserved under any h
    sizes = run_rounds(sg, g, h, s0, [(0, 1), (3, 2)])
    assert max(sizes) >= 3
    k = cr.seed_index(SEED, 0, 0, int(np.count_nonzero(s0[0] != s0[1])))
    assert cr.levels(*g, s0[0], s0[1], k) >= 2


def test_ring_one_arc_walked_from_its_end(sg):
    """150 breadth-first levels: the only differing sites are one arc, and a round is taken whose draw is the arc's end."""
    n, rng = 300, np.random.RandomState(2)
    g = ring(n, rng)
    s0 = random_spins(2, n, rng)
    s0[1] = s0[0]
    s0[1, 100:250] = -s0[0, 100:250]
    rnd = next(r for r in range(10 ** 5) if cr.seed_index(SEED, r, 0, 150) in (0, 149))
    assert cr.levels(*g, s0[0], s0[1], cr.seed_index(SEED, rnd, 0, 150)) == 150
    sizes = run_rounds(sg, g, np.zeros(n, np.float32), s0, [(1, 0)], rounds=(rnd, rnd + 1))
    assert sizes == [150, 150]


@pytest.mark.parametrize("n", [33, 65])
def test_path_component_across_a_word_edge(sg, n):
    rng = np.random.RandomState(n)
    g = path(n, rng)
    s0 = random_spins(2, n, rng)
    s0[1] = s0[0]
    s0[1, 20:] = -s0[0, 20:]  # one component over sites 20 ... n - 1: across bit 31 | 32 (and 63 | 64)
    s0[1, 3] = -s0[0, 3]      # and a lone site
    sizes = run_rounds(sg, g, np.zeros(n, np.float32), s0, [(0, 1)], rounds=ROUNDS + (5, 6, 7))
    assert set(sizes) <= {1, n - 20} and n - 20 in sizes


def test_torus(sg):
    rng = np.random.RandomState(3)
    g = torus(8, rng)
    s0 = random_spins(6, 64, rng)
    h = rng.randint(-2, 3, 64).astype(np.float32)
    run_rounds(sg, g, h, s0, [(0, 5), (2, 1), (4, 3)])


def test_star_a_row_longer_than_a_wave(sg):
    n, rng = 201, np.random.RandomState(4)
    g = star(200, rng)
    s0 = random_spins(4, n, rng)
    s0[1] = s0[0]
    s0[1, :151] = -s0[0, :151]     # the hub and 150 leaves differ: one component of 151 sites
    s0[3] = s0[2]
    s0[3, 1:120] = -s0[2, 1:120]   # the hub agrees: every differing leaf is a component of its own
    sizes = run_rounds(sg, g, np.zeros(n, np.float32), s0, [(0, 1), (2, 3)])
    assert sizes == [151, 1] * len(ROUNDS)


def test_random_graph_giant_component(sg):
    n, rng = 1000, np.random.RandomState(5)
    g = random_graph(n, 3, rng)  # degree about 6
    s0 = random_spins(4, n, rng)
    sizes = run_rounds(sg, g, rng.randint(-1, 2, n).astype(np.float32), s0, [(0, 1), (2, 3)])
    assert max(sizes) > 200  # the differing half of a degree-6 graph percolates: many words, all four waves


def test_smallest_sizes(sg):
    g1 = (np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))  # n = 1, no entries
    assert run_rounds(sg, g1, np.ones(1, np.float32), np.asarray([[1], [-1]], np.int8), [(0, 1)]) == [1, 1, 1]
    g2 = csr_from_edges(2, [(0, 1, -1.0)])
    assert run_rounds(sg, g2, np.asarray([1, -2], np.float32), np.asarray([[1, -1], [-1, 1]], np.int8), [(1, 0)]) == [2, 2, 2]
    assert run_rounds(sg, g2, np.zeros(2, np.float32), np.asarray([[1, -1], [1, 1]], np.int8), [(0, 1)]) == [1, 1, 1]


def test_opposite_replicas_flip_everything_and_identical_ones_nothing(sg):
    rng = np.random.RandomState(6)
    g = torus(8, rng)
    s0 = random_spins(4, 64, rng)
    s0[1] = -s0[0]  # connected graph, every site differs: the cluster is all n sites, the two replicas trade places
    s0[3] = s0[2]   # identical: size 0, nothing written
    h = rng.randint(-1, 2, 64).astype(np.float32)
    with engine(sg, g, h, s0) as e:
        before = state(e)
        sizes = e.cluster_move_pairs([(0, 1), (2, 3)], round=4)
        assert sizes.tolist() == [64, 0]
        now, _ = check_move(e, g, h, [(0, 1), (2, 3)], 4, SEED, before, sizes)
        assert np.array_equal(now["S"][0], s0[1]) and np.array_equal(now["S"][1], s0[0])
        assert np.array_equal(now["S"][2:], s0[2:]) and np.array_equal(now["E"][2:], before["E"][2:])
        assert np.array_equal(now["acc"][2:], before["acc"][2:])


def test_stored_zeros_do_not_connect(sg):
    n, rng = 40, np.random.RandomState(7)
    g = path(n, rng, zero_bonds=(9, 33))  # explicit 0.0 entries between sites 9 | 10 and 33 | 34
    assert np.count_nonzero(g[2] == 0) == 4
    s0 = random_spins(2, n, rng)
    s0[1] = -s0[0]
    sizes = run_rounds(sg, g, np.zeros(n, np.float32), s0, [(0, 1)], rounds=ROUNDS + tuple(range(3, 12)))
    assert set(sizes) <= {10, 24, 6} and len(set(sizes)) >= 2


def test_global_ids_and_a_small_seed(sg):
    """R_global > R_local with replica0 = 17: the draw's coordinate is the GLOBAL id of the pair's smaller replica."""
    rng = np.random.RandomState(8)
    g = torus(8, rng)
    s0 = random_spins(6, 64, rng)
    h = np.zeros(64, np.float32)
    pairs = [(4, 1), (0, 2), (3, 5)]
    run_rounds(sg, g, h, s0, pairs, seed=77, R_global=40, replica0=17)
    # the local index would give other clusters: the counts of differing sites are large enough for the draws to differ
    counts = [int(np.count_nonzero(s0[a] != s0[b])) for a, b in pairs]
    assert any(cr.seed_index(77, r, 17 + min(a, b), c) != cr.seed_index(77, r, min(a, b), c)
               for r in ROUNDS for (a, b), c in zip(pairs, counts))


def test_several_pairs_host_and_device_sizes(sg):
    n, rng = 300, np.random.RandomState(9)
    g = random_graph(n, 2, rng)
    s0 = random_spins(9, n, rng)
    h = rng.randint(-1, 2, n).astype(np.float32)
    pairs = [(8, 0), (1, 7), (2, 6), (5, 3)]  # (replica 4 is in no pair)
    with engine(sg, g, h, s0) as e:
        before = state(e)
        sizes = e.cluster_move_pairs(pairs, round=11)
        before, _ = check_move(e, g, h, pairs, 11, SEED, before, sizes)
        dev = torch.full((len(pairs),), -1, dtype=torch.int32, device="cuda")
        assert e.cluster_move_pairs(pairs, round=12, sizes=dev) is dev
        torch.cuda.synchronize()
        before, _ = check_move(e, g, h, pairs, 12, SEED, before, dev.cpu().numpy())
        assert e.cluster_move_pairs(pairs, round=13, sizes=False) is None
        S = before["S"].copy()
        want = [cr.move(*g, S[a], S[b], SEED, 13, min(a, b))[2].size for a, b in pairs]
        before, _ = check_move(e, g, h, pairs, 13, SEED, before, want)
        # round=None: the engine's exchange-round counter, which the calls leave alone
        assert e.counters() == (0, 0)
        sizes = e.cluster_move_pairs(pairs[:2])
        check_move(e, g, h, pairs[:2], 0, SEED, before, sizes)
        assert e.counters() == (0, 0)
        assert e.cluster_move_pairs(np.zeros((0, 2), np.int32)).size == 0  # no pair: a no-op


def test_a_sparse_matrix_handed_over_dense(sg):
    """sga_set_dense keeps a sparse integer matrix of n >= 4096 as CSR: the move serves it."""
    n, rng = 4096, np.random.RandomState(10)
    g = ring(n, rng)
    J = np.zeros((n, n), np.float32)
    for i in range(n):
        J[i, g[1][g[0][i]:g[0][i + 1]]] = g[2][g[0][i]:g[0][i + 1]]
    s0 = random_spins(2, n, rng)
    h = np.zeros(n, np.float32)
    with sg.AnnealEngine(0) as e:
        e.set_dense(J, h)
        e.init_replicas(2, seed=SEED, s0=s0)
        # (a dense engine would refuse the call: that it runs shows the rows were kept as CSR)
        before = state(e)
        sizes = e.cluster_move_pairs([(0, 1)], round=1)
        check_move(e, g, h, [(0, 1)], 1, SEED, before, sizes)
    # 64-bit extents (sga_set_csr64)
    with engine(sg, (g[0].astype(np.int64), g[1], g[2]), h, s0) as e:
        before = state(e)
        sizes = e.cluster_move_pairs([(1, 0)], round=2)
        check_move(e, g, h, [(1, 0)], 2, SEED, before, sizes)


# ---- 2. the ladder form --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ladders", [2, 4])
def test_ladder_form_reads_the_slot_map(sg, n_ladders):
    L, n, rng = 6, 64, np.random.RandomState(20 + n_ladders)
    g = torus(8, rng)
    h = rng.randint(-1, 2, n).astype(np.float32)
    R = n_ladders * L
    temps = np.tile(np.geomspace(4.0, 0.8, L), n_ladders)
    with engine(sg, g, h, random_spins(R, n, rng)) as e:
        e.set_ladder(temps, n_ladders)
        for _ in range(4):  # so that the slot map is a permutation of its own
            e.sweep(2)
            e.exchange()
        sm = e.slot_map()
        assert not np.array_equal(sm, np.arange(R))
        T, stats, counters = e.temperatures(), e.exchange_stats(), e.counters()
        before = state(e)
        pairs = [(int(sm[2 * c * L + s]), int(sm[(2 * c + 1) * L + s])) for c in range(n_ladders // 2) for s in range(2, 5)]
        assert all(T[a] == T[b] for a, b in pairs)  # equal slots of identical ladders: equal temperatures
        sizes = e.cluster_move_ladders(2, 5)
        assert sizes.shape == (n_ladders // 2, 3) and sizes.dtype == np.int32
        # round=None is the exchange-round counter: 4 after four exchanges
        assert counters == (8, 4)
        before, _ = check_move(e, g, h, pairs, 4, SEED, before, sizes)
        assert np.array_equal(e.slot_map(), sm) and np.array_equal(e.temperatures(), T) and e.counters() == counters
        assert all(np.array_equal(x, y) for x, y in zip(e.exchange_stats(), stats))
        # every slot, an explicit round, sizes on the device
        pairs = [(int(sm[2 * c * L + s]), int(sm[(2 * c + 1) * L + s])) for c in range(n_ladders // 2) for s in range(L)]
        dev = torch.zeros(len(pairs), dtype=torch.int32, device="cuda")
        e.cluster_move_ladders(round=2 ** 32 - 1, sizes=dev)
        torch.cuda.synchronize()
        check_move(e, g, h, pairs, 2 ** 32 - 1, SEED, before, dev.cpu().numpy())
        assert e.cluster_move_ladders(3, 3).size == 0  # an empty range: a no-op


# ---- 3. no stale state ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", ["on", "off"])
def test_sweeps_after_a_cluster_call_equal_a_fresh_engine(sg, cache):
    n, R, rng = 256, 4, np.random.RandomState(30)
    g = torus(16, rng)
    h = rng.randint(-1, 2, n).astype(np.float32)
    temps = np.asarray([1.5, 1.5, 0.7, 0.7])
    with engine(sg, g, h, random_spins(R, n, rng), cache=cache) as a:
        a.set_temperatures(temps)
        a.sweep(4)
        sizes = a.cluster_move_pairs([(0, 1), (2, 3)], round=9)
        assert sizes.max() >= 1
        S, acc0 = a.spins(), a.stats()[0]
        sw, rd = a.counters()
        a.sweep(3)
        with engine(sg, g, h, S, cache=cache) as b:
            b.set_temperatures(a.temperatures())
            b.set_counters(sw, rd)
            b.sweep(3)
            assert np.array_equal(b.spins(), a.spins())
            assert np.array_equal(b.energies(), a.energies())
            assert np.array_equal(b.stats()[0], a.stats()[0] - acc0)
            assert np.array_equal(a.energies(), oracle_energies(g, h, a.spins()))


# ---- 4. one set of rows under many field vectors ---------------------------------------------------------------------
def test_shared_csr(sg):
    n, M, per, rng = 64, 3, 4, np.random.RandomState(40)
    g = torus(8, rng)
    H = rng.randint(-2, 3, (M, n)).astype(np.float32)
    s0 = random_spins(M * per, n, rng)
    model_of = lambda r: r // per  # noqa: E731
    with sg.AnnealEngine(0) as e:
        e.set_csr_shared(*g, H)
        e.init_replicas(M * per, seed=SEED, s0=s0)
        before = state(e)
        assert np.array_equal(before["E"], oracle_energies(g, H, s0, model_of))
        pairs = [(0, 3), (2, 1), (4, 5), (11, 8), (9, 10)]  # every pair inside one model
        for rnd in ROUNDS:
            sizes = e.cluster_move_pairs(pairs, round=rnd)
            before, _ = check_move(e, g, H, pairs, rnd, SEED, before, sizes, model_of)
        with pytest.raises(sg.AnnealingError) as exc:
            e.cluster_move_pairs([(0, 1), (3, 4)], round=0)  # replicas 3 and 4 lie under two field vectors
        assert exc.value.details["code"] == sg._native.ERR_INVALID and "two models" in str(exc.value)
        now = state(e)
        assert all(np.array_equal(now[k], before[k]) for k in now)
    with sg.AnnealEngine(0) as e:
        e.set_csr_shared(*g, H[:2])
        e.init_replicas(8, seed=SEED, s0=s0[:8])
        # one ladder per model would pair replicas of two models; two per model pair inside it
        e.set_ladder(np.tile([2.0, 1.0, 0.5, 0.25], 2), 2)
        with pytest.raises(sg.AnnealingError) as exc:
            e.cluster_move_ladders(round=0)
        assert exc.value.details["code"] == sg._native.ERR_INVALID and "two models" in str(exc.value)
        e.set_ladder(np.tile([2.0, 1.0], 4), 4)
        before = state(e)
        sizes = e.cluster_move_ladders(round=3)
        check_move(e, g, H[:2], [(0, 2), (1, 3), (4, 6), (5, 7)], 3, SEED, before, sizes, model_of)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------
def refused(sg, e, code, call, *args, **kw):
    before = state(e) if e.n_models == 1 or getattr(e, "_sizes", None) is None else None
    with pytest.raises(sg.AnnealingError) as exc:
        getattr(e, call)(*args, **kw)
    assert exc.value.details["code"] == code, str(exc.value)
    if before is not None:
        now = state(e)
        assert all(np.array_equal(now[k], before[k]) for k in now)
    return str(exc.value)


def test_unsupported_problems_are_refused(sg):
    from spin_glass_anneal_rl_amd import encoders as enc
    N, rng = sg._native, np.random.RandomState(50)
    n = 48
    J = np.triu(rng.randint(0, 2, (n, n)) * 2 - 1, 1).astype(np.float32)
    with sg.AnnealEngine(0) as e:
        e.set_dense(J + J.T, np.zeros(n, np.float32))
        e.init_replicas(4, seed=1)
        assert "dense" in refused(sg, e, N.ERR_UNSUPPORTED, "cluster_move_pairs", [(0, 1)], round=0)
        e.set_ladder(np.tile([2.0, 1.0], 2), 2)
        assert "dense" in refused(sg, e, N.ERR_UNSUPPORTED, "cluster_move_ladders", round=0)
    with sg.AnnealEngine(0) as e:
        xy = rng.rand(6, 2) * 100.0
        d32, A, B, h, _ = enc.tsp_structure(np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1]), 200.0, 120.0,
                                            auto_scale=True)
        e.set_tsp(d32, A, B, h)
        e.init_replicas(2, seed=1)
        assert "sga_set_tsp" in refused(sg, e, N.ERR_UNSUPPORTED, "cluster_move_pairs", [(0, 1)], round=0)
    with sg.AnnealEngine(0) as e:
        ng, mp, mem, c, h = gc._assignment(6, 6)
        e.set_groups(ng, (mp, mem), c, h)
        e.init_replicas(2, seed=1)
        assert "sga_set_groups" in refused(sg, e, N.ERR_UNSUPPORTED, "cluster_move_pairs", [(0, 1)], round=0)
    with sg.AnnealEngine(0) as e:
        e.set_csr_batch([ring(12, rng) + (np.zeros(12, np.float32),), ring(9, rng) + (np.zeros(9, np.float32),)])
        e.init_replicas(4, seed=1)
        S, E = e.spins(), e.energies()
        assert "ragged" in refused(sg, e, N.ERR_UNSUPPORTED, "cluster_move_pairs", [(0, 1)], round=0)
        assert np.array_equal(e.spins(), S) and np.array_equal(e.energies(), E)


def test_invalid_arguments_are_refused(sg):
    N, rng = sg._native, np.random.RandomState(51)
    g = torus(8, rng)
    h = np.zeros(64, np.float32)
    with engine(sg, g, h, random_spins(6, 64, rng)) as e:
        for pairs in ([(0, 6)], [(-1, 2)], [(0, 1), (2, 0)], [(0, 1), (1, 2)], [(3, 3)], [(0, 1), (4, 4)]):
            refused(sg, e, N.ERR_INVALID, "cluster_move_pairs", pairs, round=0)
        e.set_ladder(np.tile([2.0, 1.0], 3), 3)  # an odd number of ladders
        assert "even" in refused(sg, e, N.ERR_INVALID, "cluster_move_ladders", round=0)
        e.set_ladder(np.tile([2.0, 1.0, 0.5], 2), 2)
        for lo, hi in ((-1, 2), (0, 4), (2, 1), (3, 4)):
            assert "slot range" in refused(sg, e, N.ERR_INVALID, "cluster_move_ladders", lo, hi, round=0)
        assert e.cluster_move_ladders(0, 3, round=0).shape == (1, 3)
    with engine(sg, g, h, random_spins(4, 64, rng), R_global=8, replica0=4) as e:  # a shard: the ladder form needs all replicas
        e.set_ladder(np.tile([2.0, 1.0, 0.5, 0.3], 2), 2)
        assert "R_local" in refused(sg, e, N.ERR_INVALID, "cluster_move_ladders", round=0)
    with sg.AnnealEngine(0) as e:  # no problem, then no replicas
        rc = e._lib.sga_cluster_move_pairs(e._h, np.zeros(2, np.int32).ctypes.data, 1, 0, None)
        assert rc == N.ERR_INVALID
        e.set_csr(*g, h)
        assert e._lib.sga_cluster_move_pairs(e._h, np.zeros(2, np.int32).ctypes.data, 1, 0, None) == N.ERR_INVALID
        e.init_replicas(2, seed=1)
        assert e._lib.sga_cluster_move_pairs(e._h, None, 0, 0, None) == N.ERR_INVALID      # a NULL pair list
        assert e._lib.sga_cluster_move_pairs(e._h, np.zeros(2, np.int32).ctypes.data, -1, 0, None) == N.ERR_INVALID
        assert e._lib.sga_cluster_move_pairs(None, np.zeros(2, np.int32).ctypes.data, 0, 0, None) == N.ERR_INVALID
        assert e._lib.sga_cluster_move_ladders(e._h, 0, 1, 0, None) == N.ERR_INVALID       # no ladder


# ---- 6. ParallelTempering ------------------------------------------------------------------------------------------
def pt_model(sg, rng):
    g = torus(16, rng)
    n = 256
    J = np.zeros((n, n), np.float32)
    for i in range(n):
        J[i, g[1][g[0][i]:g[0][i + 1]]] = g[2][g[0][i]:g[0][i + 1]]
    m = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=True))
    m.set_couplings_from_matrix(torch.from_numpy(J))
    return m, g


def test_parallel_tempering_with_cluster_moves(sg):
    m, g = pt_model(sg, np.random.RandomState(60))
    cfg = dict(n_replicas=6, n_sweeps=60, temp_min=0.3, temp_max=3.0, exchange_interval=5, record_interval=5, random_seed=123,
               n_copies=2, cluster_moves=True, autotune=False)
    runs = []
    for _ in range(2):
        pt = sg.ParallelTempering(sg.ParallelTemperingConfig(**cfg))
        res = pt.run(m)
        best = res.best_configuration.numpy().astype(np.int8)
        assert res.best_energy == oracle.energy(oracle.Problem(csr=g, h=np.zeros(256, np.float32)), best)
        assert pt.cluster_moves_made == 11 * 6 and pt.cluster_size_max >= 2  # eleven exchange rounds, six slots, one pair of copies
        assert pt.cluster_sites_flipped >= pt.cluster_moves_flipped >= 1
        assert len(res.energy_history) == 12 and pt.final_spins.shape == (6, 256) and pt.replica_overlaps().shape == (6, 6)
        runs.append((res.best_energy, best, list(res.energy_history), pt.cluster_sites_flipped, pt.cluster_size_max,
                     pt.exchange_accepts.copy(), pt.final_spins.copy()))
    assert all(np.array_equal(x, y) for x, y in zip(*runs))
    # the cold half only: slots at or below the temperature
    pt = sg.ParallelTempering(sg.ParallelTemperingConfig(**dict(cfg, cluster_temp_max=1.0)))
    cold = int(np.count_nonzero(np.asarray(pt.temperatures) <= 1.0))
    assert 0 < cold < 6
    pt.run(m)
    assert pt.cluster_moves_made == 11 * cold
    # copies without the moves; a model the engine refuses carries its message
    pt = sg.ParallelTempering(sg.ParallelTemperingConfig(**dict(cfg, cluster_moves=False, n_copies=3)))
    res = pt.run(m)
    assert pt.cluster_moves_made == 0
    assert res.best_energy == oracle.energy(oracle.Problem(csr=g, h=np.zeros(256, np.float32)), res.best_configuration.numpy().astype(np.int8))
    dense = sg.IsingModel(sg.IsingModelConfig(n_spins=16, use_sparse=False))
    rng = np.random.RandomState(61)
    J = np.triu(rng.randint(0, 2, (16, 16)) * 2 - 1, 1).astype(np.float32)
    dense.set_couplings_from_matrix(torch.from_numpy(J + J.T))
    with pytest.raises(sg.ConfigurationError, match="dense"):
        sg.ParallelTempering(sg.ParallelTemperingConfig(**cfg)).run(dense)
