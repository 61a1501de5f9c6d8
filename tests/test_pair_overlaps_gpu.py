"""Spin and link overlaps between pairs of replicas on the device (sga_get_link_count / sga_get_pair_overlaps /
sga_accumulate_ladder_overlaps, csrc/pair_overlaps.hip).  Every number is an integer count, so every comparison is
np.array_equal against tests/overlap_reference.py: distances, broken links, link counts, the histograms of the ladder
form fed with the slot map of each round.  Spins come in through s0 and couplings are +-1 unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest
import torch

import groups_cases as gc
import overlap_reference as ovr
from test_cluster_moves_gpu import SEED, csr_from_edges, path, pm, random_graph, random_spins, ring, star, state, torus

pytestmark = pytest.mark.gpu

R6 = 6
PAIRS = [(a, b) for a in range(R6) for b in range(a + 1, R6)] + [(2, 2)]  # all 15 pairs of six replicas, and a == b


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def complete(n, rng):
    return csr_from_edges(n, [(i, j, pm(rng)) for i in range(n) for j in range(i + 1, n)])


def one_site():
    return np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)


def with_diagonal(rng):
    """A ring of 9 with a stored diagonal entry in rows 0 and 4 (rows sorted by column)."""
    rowptr, col, val = ring(9, rng)
    rows = [list(zip(col[rowptr[i]:rowptr[i + 1]], val[rowptr[i]:rowptr[i + 1]])) for i in range(9)]
    rows[0].append((0, 2.0))
    rows[4].append((4, -1.0))
    rows = [sorted(r) for r in rows]
    return (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32),
            np.asarray([j for r in rows for j, _ in r], np.int32), np.asarray([v for r in rows for _, v in r], np.float32))


GRAPHS = {
    "one-site": lambda rng: one_site(),
    "ring-12": lambda rng: ring(12, rng),
    "ring-32": lambda rng: ring(32, rng),   # the bitmap's word edges
    "ring-33": lambda rng: ring(33, rng),
    "torus-6x6": lambda rng: torus(6, rng),
    "star-300": lambda rng: star(300, rng),  # a hub row longer than any lane group, beside leaves of one entry
    "random-70": lambda rng: random_graph(70, 3, rng),
    "path-stored-zeros": lambda rng: path(40, rng, zero_bonds=(9, 10, 33)),
    "diagonal-entries": with_diagonal,
    "complete-200": lambda rng: complete(200, rng),  # mean row 199: 64-entry slots with padding, a wave to a row
}


def reference(graph, S, pairs):
    return (np.asarray([ovr.dist(S[a], S[b]) for a, b in pairs], np.int32),
            np.asarray([ovr.broken(*graph, S[a], S[b]) for a, b in pairs], np.int64))


def check_pairs(e, graph, S, pairs=PAIRS, which="current"):
    want_d, want_b = reference(graph, S, pairs)
    d, b = e.pair_overlaps(pairs, which=which)
    assert d.dtype == np.int32 and b.dtype == np.int64
    assert np.array_equal(d, want_d)
    assert np.array_equal(b, want_b)
    d2, none = e.pair_overlaps(pairs, which=which, links=False)
    assert none is None and np.array_equal(d2, want_d)
    return want_d, want_b


def make(sg, graph, s0, h=None, options=None, cache=None, wide=False, **replicas):
    e = sg.AnnealEngine(0)
    for k, v in (options or {}).items():
        e.set_option(k, v)
    if cache is not None:
        e.set_field_cache(cache)
    n = len(graph[0]) - 1
    rowptr = graph[0].astype(np.int64) if wide else graph[0]
    e.set_csr(rowptr, graph[1], graph[2], np.zeros(n, np.float32) if h is None else h)
    e.init_replicas(len(s0), seed=SEED, s0=s0, **replicas)
    return e


# ---- 1. the pair form and the link count against the reference -------------------------------------------------------
@pytest.mark.parametrize("name", list(GRAPHS))
def test_graphs(sg, name):
    rng = np.random.RandomState(sorted(GRAPHS).index(name))
    g = GRAPHS[name](rng)
    n = len(g[0]) - 1
    S = random_spins(R6, n, rng)
    S[5] = -S[4]  # every site differs: d = n, no link broken
    with make(sg, g, S) as e:
        assert e.link_count() == ovr.link_count(*g)
        want_d, want_b = check_pairs(e, g, S)
        assert want_d[PAIRS.index((4, 5))] == n and want_b[PAIRS.index((4, 5))] == 0 and want_d[-1] == 0 and want_b[-1] == 0
        if name not in ("one-site",):
            assert want_b.max() > 0
    if name == "path-stored-zeros":
        assert np.count_nonzero(g[2] == 0) == 6 and ovr.link_count(*g) == len(g[2]) - 6
    if name == "diagonal-entries":
        assert ovr.link_count(*g) == len(g[2]) - 2


def test_zero_slots_inside_the_layout(sg):
    """Option zero_slot_every = 1: an all-zero slot behind every row's slots -- padding the walk passes over."""
    rng = np.random.RandomState(11)
    g = complete(200, rng)
    S = random_spins(R6, 200, rng)
    with make(sg, g, S, options={"zero_slot_every": 1}) as e:
        assert e.link_count() == 200 * 199
        check_pairs(e, g, S)


def test_wide_extents_and_a_sparse_matrix_handed_over_dense(sg):
    rng = np.random.RandomState(12)
    g = ring(12, rng)
    S = random_spins(R6, 12, rng)
    with make(sg, g, S, wide=True) as e:  # sga_set_csr64
        assert e.link_count() == 24
        check_pairs(e, g, S)
    # sga_set_dense keeps a sparse integer matrix of n >= 4096 as CSR
    n = 4096
    g = ring(n, rng)
    J = np.zeros((n, n), np.float32)
    for i in range(n):
        J[i, g[1][g[0][i]:g[0][i + 1]]] = g[2][g[0][i]:g[0][i + 1]]
    S = random_spins(R6, n, rng)
    with sg.AnnealEngine(0) as e:
        e.set_dense(J, np.zeros(n, np.float32))
        e.init_replicas(R6, seed=SEED, s0=S)
        assert e.link_count() == 2 * n  # (a dense engine would refuse: the rows were kept as CSR)
        check_pairs(e, g, S)


def test_shared_csr_a_pair_across_two_field_vectors(sg):
    rng = np.random.RandomState(13)
    g = torus(6, rng)
    H = rng.randint(-2, 3, (2, 36)).astype(np.float32)
    S = random_spins(R6, 36, rng)
    with sg.AnnealEngine(0) as e:
        e.set_csr_shared(*g, H)
        e.init_replicas(R6, seed=SEED, s0=S)
        assert e.link_count() == 4 * 36
        check_pairs(e, g, S)  # (2, 3), (0, 5) ... join replicas under the two field vectors: the graph is one


def test_outputs_on_the_device_and_many_pairs(sg):
    rng = np.random.RandomState(14)
    g = random_graph(70, 3, rng)
    S = random_spins(R6, 70, rng)
    pairs = [(int(a), int(b)) for a, b in rng.randint(0, R6, (300, 2))]  # more pairs than replicas: a replica in many
    want_d, want_b = reference(g, S, pairs)
    with make(sg, g, S) as e:
        d = torch.full((300,), -1, dtype=torch.int32, device="cuda")
        b = torch.full((300,), -1, dtype=torch.int64, device="cuda")
        got = e.pair_overlaps(pairs, dist=d, broken=b)
        assert got[0] is d and got[1] is b
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), want_d) and np.array_equal(b.cpu().numpy(), want_b)
        # one output on the host, one on the device; one output alone
        b.fill_(-1)
        torch.cuda.synchronize()
        dh, bd = e.pair_overlaps(pairs, broken=b)
        torch.cuda.synchronize()
        assert np.array_equal(dh, want_d) and np.array_equal(bd.cpu().numpy(), want_b)
        hb = np.zeros(300, np.int64)
        pr = np.ascontiguousarray(pairs, np.int32)
        assert e._lib.sga_get_pair_overlaps(e._h, 0, pr.ctypes.data_as(C.c_void_p), 300, None, hb.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(hb, want_b)
        assert all(x.size == 0 for x in e.pair_overlaps(np.zeros((0, 2), np.int32)))  # no pair: a no-op


# ---- 2. the rows in HBM are what is measured ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["cache-on", "bit-spins", "plain"])
def test_current_and_best_after_sweeps(sg, form):
    rng = np.random.RandomState(20)
    g = torus(6, rng)
    S0 = random_spins(R6, 36, rng)
    opts = {"force_csr_bits": 1} if form == "bit-spins" else None
    with make(sg, g, S0, options=opts, cache="on" if form == "cache-on" else "off") as e:
        e.set_temperatures(np.geomspace(3.0, 0.5, R6))
        e.sweep(10)
        S = e.spins()
        assert not np.array_equal(S, S0)
        check_pairs(e, g, S)
        best = np.stack([e.best(r)[1] for r in range(R6)])
        assert not np.array_equal(best, S)
        check_pairs(e, g, best, which="best")


# ---- 3. what has no stored rows gets the spin part alone ---------------------------------------------------------------
def refused(sg, code, fn, *args, **kw):
    with pytest.raises(sg.AnnealingError) as exc:
        fn(*args, **kw)
    assert exc.value.details["code"] == code, str(exc.value)
    return str(exc.value)


def spin_part_only(sg, e, word):
    """dist against overlaps(); broken, hist_l and link_count() refused with the reason."""
    N = sg._native
    n, R = e.n, e.R
    pairs = [(a, b) for a in range(R) for b in range(R)]
    Q = e.overlaps()
    d, none = e.pair_overlaps(pairs, links=False)
    assert none is None and np.array_equal(d, np.asarray([(n - Q[a, b]) // 2 for a, b in pairs], np.int32))
    assert np.array_equal(d, np.asarray([ovr.dist(e.spins(a), e.spins(b)) for a, b in pairs], np.int32))
    assert word in refused(sg, N.ERR_UNSUPPORTED, e.link_count)
    assert word in refused(sg, N.ERR_UNSUPPORTED, e.pair_overlaps, pairs)
    e.set_ladder(np.tile(np.geomspace(2.0, 1.0, R // 2), 2), 2)
    hq = torch.zeros((1, R // 2, n + 1), dtype=torch.int64, device="cuda")
    hl = torch.zeros((1, R // 2, 8), dtype=torch.int64, device="cuda")
    assert word in refused(sg, N.ERR_UNSUPPORTED, e.accumulate_ladder_overlaps, hq, hl)
    torch.cuda.synchronize()
    assert int(hq.sum()) == 0 and int(hl.sum()) == 0
    e.accumulate_ladder_overlaps(hq)
    torch.cuda.synchronize()
    want = np.zeros((1, R // 2, n + 1), np.int64)
    ovr.accumulate(want, None, e.slot_map(), R // 2, None, e.spins())
    assert np.array_equal(hq.cpu().numpy(), want)


def test_dense_groups_tsp_and_ragged_engines(sg):
    from spin_glass_anneal_rl_amd import encoders as enc
    rng = np.random.RandomState(30)
    n = 40
    J = np.triu(rng.randint(0, 2, (n, n)) * 2 - 1, 1).astype(np.float32)
    with sg.AnnealEngine(0) as e:
        e.set_dense(J + J.T, np.zeros(n, np.float32))
        e.init_replicas(4, seed=1)
        spin_part_only(sg, e, "dense")
    with sg.AnnealEngine(0) as e:
        ng, mp, mem, c, h = gc._assignment(6, 6)
        e.set_groups(ng, (mp, mem), c, h)
        e.init_replicas(4, seed=1)
        spin_part_only(sg, e, "sga_set_groups")
    with sg.AnnealEngine(0) as e:
        xy = rng.rand(6, 2) * 100.0
        d32, A, B, h, _ = enc.tsp_structure(np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1]), 200.0, 120.0,
                                            auto_scale=True)
        e.set_tsp(d32, A, B, h)
        e.init_replicas(4, seed=1)
        spin_part_only(sg, e, "sga_set_tsp")
    with sg.AnnealEngine(0) as e:  # ragged rows are zero past a model's own sites and never differ there
        e.set_csr_batch([ring(12, rng) + (np.zeros(12, np.float32),), ring(9, rng) + (np.zeros(9, np.float32),)])
        e.init_replicas(4, seed=1)
        S = e.spins()
        d, _ = e.pair_overlaps([(0, 1), (2, 3)], links=False)
        assert d.tolist() == [ovr.dist(S[0][:12], S[1][:12]), ovr.dist(S[2][:9], S[3][:9])]
        assert "ragged" in refused(sg, sg._native.ERR_UNSUPPORTED, e.link_count)
        assert "ragged" in refused(sg, sg._native.ERR_UNSUPPORTED, e.pair_overlaps, [(0, 1)])


# ---- 4. the ladder form ----------------------------------------------------------------------------------------------
def test_ladder_form_histograms(sg):
    n_ladders, L, n, rounds = 4, 5, 36, 3
    rng = np.random.RandomState(40)
    g = torus(6, rng)
    links = ovr.link_count(*g)
    assert links == 144
    R = n_ladders * L
    P = n_ladders // 2
    #            name          (lo, hi)  q_shift l_shift bins_q  bins_l
    variants = {"exact":      ((0, L),   0,      0,      n + 1,  links + 1),
                "clamped":    ((0, L),   2,      3,      3,      3),
                "slot-range": ((1, 4),   0,      0,      n + 1,  links + 1),
                "spins-only": ((0, L),   0,      0,      n + 1,  None)}
    dev, ref = {}, {}
    for name, ((lo, hi), qs, ls, bq, bl) in variants.items():
        dev[name] = (torch.zeros((P, hi - lo, bq), dtype=torch.int64, device="cuda"),
                     None if bl is None else torch.zeros((P, hi - lo, bl), dtype=torch.int64, device="cuda"))
        ref[name] = (np.zeros((P, hi - lo, bq), np.int64), None if bl is None else np.zeros((P, hi - lo, bl), np.int64))
    with make(sg, g, random_spins(R, n, rng)) as e:
        e.set_ladder(np.tile(np.geomspace(4.0, 0.8, L), n_ladders), n_ladders)
        assert e.link_count() == links
        for _ in range(rounds):
            e.sweep(2)
            e.exchange()
            sm, S = e.slot_map(), e.spins()
            for name, ((lo, hi), qs, ls, bq, bl) in variants.items():
                assert e.accumulate_ladder_overlaps(dev[name][0], dev[name][1], slot_lo=lo, slot_hi=hi, q_shift=qs, l_shift=ls) is None
                ovr.accumulate(ref[name][0], ref[name][1], sm, L, g, S, slot_lo=lo, slot_hi=hi, q_shift=qs, l_shift=ls)
        assert not np.array_equal(sm, np.arange(R))  # the exchanges permuted the slot map
        assert e._lib.sga_accumulate_ladder_overlaps(e._h, 2, 2, C.c_void_p(dev["exact"][0].data_ptr()), n + 1, 0, None, 0, 0) == 0  # an empty range: a no-op
        torch.cuda.synchronize()
        for name, ((lo, hi), *_rest) in variants.items():
            for got, want in zip(dev[name], ref[name]):
                if want is None:
                    assert got is None
                    continue
                got = got.cpu().numpy()
                assert np.array_equal(got, want), name
                assert got.sum() == rounds * P * (hi - lo), name
                assert np.array_equal(got.sum(axis=2), np.full((P, hi - lo), rounds)), name  # one count per cell and call
    assert ref["clamped"][0][:, :, 2].sum() > 0 and ref["clamped"][1][:, :, 2].sum() > 0  # the clamp was exercised


# ---- 5. refusals leave the histograms and the outputs untouched --------------------------------------------------------
def test_invalid_arguments_are_refused(sg):
    N, rng = sg._native, np.random.RandomState(50)
    g = torus(6, rng)
    n = 36
    with make(sg, g, random_spins(6, n, rng)) as e:
        lib, h = e._lib, e._h
        hq = torch.full((1, 3, n + 1), 7, dtype=torch.int64, device="cuda")
        hl = torch.full((1, 3, 145), 7, dtype=torch.int64, device="cuda")
        d = torch.full((2,), -5, dtype=torch.int32, device="cuda")
        b = torch.full((2,), -5, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        qp, lp = C.c_void_p(hq.data_ptr()), C.c_void_p(hl.data_ptr())
        # no ladder yet
        assert lib.sga_accumulate_ladder_overlaps(h, 0, 1, qp, n + 1, 0, lp, 145, 0) == N.ERR_INVALID
        assert "no ladder" in N.last_error()
        e.set_ladder(np.tile([2.0, 1.0], 3), 3)  # an odd number of ladders
        assert "even" in refused(sg, N.ERR_INVALID, e.accumulate_ladder_overlaps, torch.zeros((1, 2, 4), dtype=torch.int64, device="cuda"))
        e.set_ladder(np.tile([2.0, 1.0, 0.5], 2), 2)
        for lo, hi in ((-1, 2), (0, 4), (2, 1), (3, 4)):
            assert lib.sga_accumulate_ladder_overlaps(h, lo, hi, qp, n + 1, 0, lp, 145, 0) == N.ERR_INVALID
        host = np.full((1, 3, n + 1), 7, np.int64)
        assert lib.sga_accumulate_ladder_overlaps(h, 0, 3, host.ctypes.data_as(C.c_void_p), n + 1, 0, None, 0, 0) == N.ERR_INVALID  # a host hist_q
        assert lib.sga_accumulate_ladder_overlaps(h, 0, 3, qp, n + 1, 0, host.ctypes.data_as(C.c_void_p), n + 1, 0) == N.ERR_INVALID
        assert lib.sga_accumulate_ladder_overlaps(h, 0, 3, None, n + 1, 0, None, 0, 0) == N.ERR_INVALID
        assert lib.sga_accumulate_ladder_overlaps(h, 0, 3, qp, 0, 0, None, 0, 0) == N.ERR_INVALID      # bins_q = 0
        assert lib.sga_accumulate_ladder_overlaps(h, 0, 3, qp, n + 1, 0, lp, 0, 0) == N.ERR_INVALID    # bins_l = 0
        assert lib.sga_accumulate_ladder_overlaps(h, 0, 3, qp, n + 1, 32, None, 0, 0) == N.ERR_INVALID  # shift 32
        assert lib.sga_accumulate_ladder_overlaps(h, 0, 3, qp, n + 1, 0, lp, 145, -1) == N.ERR_INVALID
        assert lib.sga_accumulate_ladder_overlaps(None, 0, 3, qp, n + 1, 0, None, 0, 0) == N.ERR_INVALID
        refused(sg, N.ERR_INVALID, e.accumulate_ladder_overlaps, hq, hl, q_shift=32)
        # the pair form
        for pairs in ([(0, 1), (0, 6)], [(-1, 2), (0, 1)]):  # an index R, an index -1
            refused(sg, N.ERR_INVALID, e.pair_overlaps, pairs, dist=d, broken=b)
        pr = np.asarray([[0, 1], [2, 3]], np.int32)
        pp = pr.ctypes.data_as(C.c_void_p)
        dp, bp = C.c_void_p(d.data_ptr()), C.c_void_p(b.data_ptr())
        assert lib.sga_get_pair_overlaps(h, 0, pp, 2, None, None) == N.ERR_INVALID   # both outputs NULL
        assert lib.sga_get_pair_overlaps(h, 2, pp, 2, dp, bp) == N.ERR_INVALID       # which outside {0, 1}
        assert lib.sga_get_pair_overlaps(h, -1, pp, 2, dp, bp) == N.ERR_INVALID
        assert lib.sga_get_pair_overlaps(h, 0, pp, -1, dp, bp) == N.ERR_INVALID      # count < 0
        assert lib.sga_get_pair_overlaps(h, 0, None, 2, dp, bp) == N.ERR_INVALID     # a NULL list with count > 0
        assert lib.sga_get_pair_overlaps(None, 0, pp, 2, dp, bp) == N.ERR_INVALID
        assert lib.sga_get_pair_overlaps(h, 0, None, 0, dp, bp) == N.OK  # count == 0: a no-op
        assert lib.sga_get_link_count(h, None) == N.ERR_INVALID
        torch.cuda.synchronize()
        assert bool((hq == 7).all()) and bool((hl == 7).all()) and np.all(host == 7)
        assert bool((d == -5).all()) and bool((b == -5).all())
        # and the calls still work
        e.accumulate_ladder_overlaps(hq, hl)
        torch.cuda.synchronize()
        assert int(hq.sum()) == 7 * hq.numel() + 3 and int(hl.sum()) == 7 * hl.numel() + 3
    with make(sg, g, random_spins(4, n, rng), R_global=8, replica0=4) as e:  # a shard: the ladder form needs all replicas
        e.set_ladder(np.tile([2.0, 1.0, 0.5, 0.3], 2), 2)
        assert "R_local" in refused(sg, N.ERR_INVALID, e.accumulate_ladder_overlaps, torch.zeros((1, 4, 4), dtype=torch.int64, device="cuda"))
        d_, b_ = e.pair_overlaps([(0, 3)])  # the pair form takes local indices on a shard
        S = e.spins()
        assert d_[0] == ovr.dist(S[0], S[3]) and b_[0] == ovr.broken(*g, S[0], S[3])
    with sg.AnnealEngine(0) as e:  # no problem, then no replicas
        out = np.zeros(1, np.int64)
        pr = np.zeros(2, np.int32)
        dd = np.full(1, -5, np.int32)
        for _ in range(2):
            assert e._lib.sga_get_link_count(e._h, out.ctypes.data_as(C.c_void_p)) == N.ERR_INVALID
            assert e._lib.sga_get_pair_overlaps(e._h, 0, pr.ctypes.data_as(C.c_void_p), 1, dd.ctypes.data_as(C.c_void_p), None) == N.ERR_INVALID
            e.set_csr(*g, np.zeros(n, np.float32))
        assert dd[0] == -5 and out[0] == 0


# ---- 6. nothing moves ------------------------------------------------------------------------------------------------
def test_a_run_with_the_calls_interleaved_walks_the_same_chain(sg):
    n_ladders, L, n = 2, 4, 36
    rng = np.random.RandomState(60)
    g = torus(6, rng)
    h = rng.randint(-1, 2, n).astype(np.float32)
    s0 = random_spins(n_ladders * L, n, rng)
    temps = np.tile(np.geomspace(3.0, 0.6, L), n_ladders)
    hq = torch.zeros((1, L, n + 1), dtype=torch.int64, device="cuda")
    hl = torch.zeros((1, L, 145), dtype=torch.int64, device="cuda")
    pairs = [(0, 7), (3, 3), (5, 1)]
    with make(sg, g, s0, h=h, cache="on") as a, make(sg, g, s0, h=h, cache="on") as b:
        for e in (a, b):
            e.set_ladder(temps, n_ladders)
        for k in range(20):
            a.sweep(1)
            b.sweep(1)
            kernel = b.last_kernel()
            b.pair_overlaps(pairs)
            b.pair_overlaps(pairs, which="best", links=False)
            b.accumulate_ladder_overlaps(hq, hl)
            assert b.link_count() == 144
            assert b.last_kernel() == kernel
            if k % 2 == 1:
                a.exchange()
                b.exchange()
        sa, sb = state(a), state(b)
        assert all(np.array_equal(sa[k], sb[k]) for k in sa)  # spins, energies, accept counters, bests
        assert np.array_equal(a.slot_map(), b.slot_map()) and a.counters() == b.counters() == (20, 10)
        assert all(np.array_equal(x, y) for x, y in zip(a.exchange_stats(), b.exchange_stats()))
        assert np.array_equal(a.stats()[1], b.stats()[1]) and a.last_kernel() == b.last_kernel()
        assert np.array_equal(a.temperatures(), b.temperatures())
        torch.cuda.synchronize()
        assert int(hq.sum()) == 20 * L and int(hl.sum()) == 20 * L


# ---- 7. ParallelTempering --------------------------------------------------------------------------------------------
def pt_model(sg, g, n):
    J = np.zeros((n, n), np.float32)
    for i in range(n):
        J[i, g[1][g[0][i]:g[0][i + 1]]] = g[2][g[0][i]:g[0][i + 1]]
    m = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=True))
    m.set_couplings_from_matrix(torch.from_numpy(J))
    return m


def test_parallel_tempering_measures_overlaps(sg):
    g = torus(6, np.random.RandomState(70))
    m = pt_model(sg, g, 36)
    cfg = dict(n_replicas=5, n_sweeps=20, temp_min=0.4, temp_max=3.0, exchange_interval=2, record_interval=2, random_seed=321,
               n_copies=2, cluster_moves=True, autotune=False, measure_overlaps=True, measure_after=4, measure_interval=2)
    pt = sg.ParallelTempering(sg.ParallelTemperingConfig(**cfg))
    res = pt.run(m)
    st = pt.overlap_statistics
    # exchange rounds behind sweeps 2, 4 ... 18; from sweep 4 on every second one: those behind sweeps 4, 8, 12, 16
    assert pt.overlap_rounds_measured == 4
    assert st.hist_q.shape == (1, 5, 37) and st.hist_l.shape == (1, 5, 145) and st.n == 36 and st.n_links == 144
    assert st.hist_q.sum() == 4 * 5 and st.hist_l.sum() == 4 * 5
    assert np.array_equal(st.hist_q.sum(axis=2), np.full((1, 5), 4)) and (st.q_shift, st.l_shift) == (0, 0)
    assert np.array_equal(st.temperatures, np.asarray(pt.temperatures))
    q2, q4 = st.moments()
    assert q2.shape == (5,) and np.all((q2 >= 0) & (q2 <= 1)) and np.all(q4 <= q2) and np.all(np.abs(st.link_overlap()) <= 1)
    # the measurement moves nothing: the same run without it
    off = sg.ParallelTempering(sg.ParallelTemperingConfig(**dict(cfg, measure_overlaps=False)))
    res_off = off.run(m)
    assert off.overlap_statistics is None and off.overlap_rounds_measured == 0
    assert res.best_energy == res_off.best_energy
    assert np.array_equal(res.best_configuration.numpy(), res_off.best_configuration.numpy())
    assert np.array_equal(pt.final_spins, off.final_spins)
    assert np.array_equal(pt.exchange_accepts, off.exchange_accepts) and np.array_equal(pt.exchange_attempts, off.exchange_attempts)
    assert res.energy_history == res_off.energy_history and pt.cluster_sites_flipped == off.cluster_sites_flipped
    # binned: at most 8 bins each
    binned = sg.ParallelTempering(sg.ParallelTemperingConfig(**dict(cfg, overlap_bins=8, measure_after=0, measure_interval=1)))
    binned.run(m)
    sb = binned.overlap_statistics
    assert binned.overlap_rounds_measured == 9 and (sb.q_shift, sb.l_shift) == (3, 5)
    assert sb.hist_q.shape == (1, 5, 5) and sb.hist_l.shape == (1, 5, 5) and sb.hist_q.sum() == 45 and sb.hist_l.sum() == 45
    # a dense model: the spin part only
    dense = sg.IsingModel(sg.IsingModelConfig(n_spins=16, use_sparse=False))
    rng = np.random.RandomState(71)
    J = np.triu(rng.randint(0, 2, (16, 16)) * 2 - 1, 1).astype(np.float32)
    dense.set_couplings_from_matrix(torch.from_numpy(J + J.T))
    ptd = sg.ParallelTempering(sg.ParallelTemperingConfig(**dict(cfg, cluster_moves=False)))
    ptd.run(dense)
    assert ptd.overlap_statistics.hist_l is None and ptd.overlap_statistics.n_links is None
    assert ptd.overlap_statistics.hist_q.shape == (1, 5, 17) and ptd.overlap_statistics.hist_q.sum() == 20
