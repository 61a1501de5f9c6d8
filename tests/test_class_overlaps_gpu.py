"""Class-resolved overlaps between pairs of replicas on the device (sga_get_class_overlaps /
sga_accumulate_ladder_class_overlaps, csrc/class_overlaps.hip).  Every number is an integer count, so every comparison is
np.array_equal against tests/class_overlap_reference.py: the pair form on the spins that went in or that spins() returns,
the sums of the ladder form fed with the slot map and spins of each round."""
import ctypes as C

import numpy as np
import pytest
import torch

import class_overlap_reference as cor
import groups_cases as gc
from test_cluster_moves_gpu import SEED, csr_from_edges, path, pm, random_spins, state, torus

pytestmark = pytest.mark.gpu

R6 = 6
PAIRS = [(a, b) for a in range(R6) for b in range(a + 1, R6)] + [(2, 2)]  # all 15 pairs of six replicas, and a == b


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def chain(n, rng):
    """A path of n sites; one site has no bond at all."""
    if n == 1:
        return np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
    return path(n, rng)


def lattice3d(L, rng):
    """The +-J lattice of L^3 sites with periodic boundaries, row-major: the matching class map is lattice_planes((L, L, L))."""
    idx = lambda x, y, z: ((x % L) * L + (y % L)) * L + (z % L)  # noqa: E731
    return csr_from_edges(L ** 3, [(idx(x, y, z), idx(x + dx, y + dy, z + dz), pm(rng)) for x in range(L) for y in range(L)
                                   for z in range(L) for dx, dy, dz in ((1, 0, 0), (0, 1, 0), (0, 0, 1))])


def make(sg, graph, s0, h=None, options=None, cache=None, **replicas):
    e = sg.AnnealEngine(0)
    for k, v in (options or {}).items():
        e.set_option(k, v)
    if cache is not None:
        e.set_field_cache(cache)
    n = len(graph[0]) - 1
    e.set_csr(graph[0], graph[1], graph[2], np.zeros(n, np.float32) if h is None else h)
    e.init_replicas(len(s0), seed=SEED, s0=s0, **replicas)
    return e


def check(e, S, classes, n_classes, pairs=PAIRS, which="current", device_map=False, device_out=False):
    """One call against the reference; returns the counts."""
    want = cor.pair_form(S, pairs, classes, n_classes)
    cl = torch.from_numpy(np.ascontiguousarray(classes, np.int32)).cuda() if device_map else classes
    out = None
    if device_out:
        out = torch.full(want.shape, -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
    got = e.class_overlaps(pairs, cl, n_classes, which=which, out=out)
    if device_out:
        assert got is out
        torch.cuda.synchronize()
        got = out.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)
    return got


# ---- 1. the pair form against the reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])  # the wave's and the workgroup's strides
def test_pair_form_sizes_and_maps(sg, n):
    rng = np.random.RandomState(n)
    S = random_spins(R6, n, rng)
    S[5] = -S[4]  # every site differs: D_c = N_c
    maps = {
        "C=1": (np.zeros(n, np.int32), 1),
        "C=2": ((np.arange(n) % 2).astype(np.int32), 2),
        "C=7": (rng.randint(0, 7, n).astype(np.int32), 7),
        "C=n": (np.arange(n, dtype=np.int32), n),                    # every site its own class
        "one-class-of-5": (np.full(n, 3, np.int32), 5),              # the greatest contention
        "blocks-of-64": ((np.arange(n) // 64).astype(np.int32), (n + 63) // 64),  # a wave's sites share one class
        "out-of-range": (rng.randint(-2, 9, n).astype(np.int32), 7),  # -2, -1, 7 and 8 are no class
        "M=3": (np.stack([rng.randint(0, 7, n), np.arange(n) % 7, np.arange(n) // 37 % 7]).astype(np.int32), 7),
        "M=3-out-of-range": (np.stack([rng.randint(-1, 6, n), np.full(n, 5), np.full(n, -1)]).astype(np.int32), 5),
    }
    with make(sg, chain(n, rng), S) as e:
        dist = e.pair_overlaps(PAIRS, links=False)[0]
        for k, (name, (classes, n_classes)) in enumerate(maps.items()):
            got = check(e, S, classes, n_classes, device_map=k % 2 == 1, device_out=k % 3 == 1)
            if "out-of-range" not in name:  # every site has a class: the counts add up to the distance
                assert np.array_equal(got.sum(axis=2), np.repeat(dist[:, None], got.shape[1], axis=1)), name
            else:
                assert np.all(got.sum(axis=2) <= dist[:, None]), name
            sizes = np.stack([np.bincount(c[(c >= 0) & (c < n_classes)], minlength=n_classes) for c in cor.maps(classes)])
            assert not got[-1].any() and np.array_equal(got[PAIRS.index((4, 5))], sizes), name  # a == b: zeros; all differ: N_c
        # ld > n: rows wider than the engine's, on the host and as a view of a wider device tensor
        wide = np.concatenate([maps["M=3"][0], rng.randint(0, 7, (3, 5)).astype(np.int32)], axis=1)
        want = cor.pair_form(S, PAIRS, maps["M=3"][0], 7)
        assert np.array_equal(e.class_overlaps(PAIRS, wide, 7), want)
        view = torch.from_numpy(wide).cuda()[:, :n]
        assert view.stride(0) == n + 5
        assert np.array_equal(e.class_overlaps(PAIRS, view, 7), want)
        # every combination of host / device map and host / device output
        for device_map in (False, True):
            for device_out in (False, True):
                check(e, S, maps["M=3"][0], 7, device_map=device_map, device_out=device_out)


def test_counter_copies_threshold_and_the_bound(sg):
    """M C on either side of the four-copy threshold, the largest product served and the first refused."""
    N, rng = sg._native, np.random.RandomState(5)
    n = 257
    S = random_spins(R6, n, rng)
    S[5] = -S[4]
    assert (cor.MAX_MC_4, cor.MAX_MC) == (10224, 40896)
    with make(sg, chain(n, rng), S) as e:
        for M, Cn in ((1, 10224), (1, 10225), (3, 3408), (3, 3409), (1, 40896), (2, 20448)):
            assert cor.copies(M * Cn) == (4 if M * Cn <= 10224 else 1)
            classes = rng.randint(0, Cn, (M, n)).astype(np.int32)
            classes[:, :3] = [0, Cn - 1, Cn]  # the first and the last counter, and one past them: no class
            got = check(e, S, classes, Cn, device_map=True)
            assert np.all(got[PAIRS.index((4, 5)), :, 0] >= 1) and np.all(got[PAIRS.index((4, 5)), :, Cn - 1] >= 1)
        for M, Cn in ((1, 40897), (3, 13633)):
            classes = torch.zeros((M, n), dtype=torch.int32, device="cuda")
            out = torch.full((2, M, Cn), -5, dtype=torch.int32, device="cuda")
            host = np.full((2, M, Cn), -5, np.int32)
            torch.cuda.synchronize()
            with pytest.raises(sg.AnnealingError) as exc:
                e.class_overlaps([(0, 1), (2, 3)], classes, Cn, out=out)
            assert exc.value.details["code"] == N.ERR_UNSUPPORTED and "40896" in str(exc.value)
            pr = np.asarray([[0, 1], [2, 3]], np.int32)
            assert e._lib.sga_get_class_overlaps(e._h, 0, pr.ctypes.data_as(C.c_void_p), 2, C.c_void_p(classes.data_ptr()), n, M, Cn,
                                                 host.ctypes.data_as(C.c_void_p)) == N.ERR_UNSUPPORTED
            torch.cuda.synchronize()
            assert bool((out == -5).all()) and np.all(host == -5)


def test_many_pairs(sg):
    rng = np.random.RandomState(14)
    n = 70
    S = random_spins(R6, n, rng)
    pairs = [(int(a), int(b)) for a, b in rng.randint(0, R6, (300, 2))]  # more pairs than replicas: a replica in many
    classes = np.stack([rng.randint(0, 4, n), np.arange(n) % 4]).astype(np.int32)
    with make(sg, chain(n, rng), S) as e:
        check(e, S, classes, 4, pairs=pairs)
        check(e, S, classes, 4, pairs=pairs, device_map=True, device_out=True)
        assert e.class_overlaps(np.zeros((0, 2), np.int32), classes, 4).shape == (0, 2, 4)  # no pair: a no-op
        assert np.array_equal(e.class_overlaps(PAIRS, classes[1], 4), cor.pair_form(S, PAIRS, classes[1:], 4))  # a map [n]


# ---- 2. the rows in HBM are what is measured ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["cache-on", "bit-spins"])
def test_current_and_best_after_sweeps(sg, form):
    rng = np.random.RandomState(20)
    g = torus(6, rng)
    S0 = random_spins(R6, 36, rng)
    planes = sg.encoders.lattice_planes((6, 6))
    opts = {"force_csr_bits": 1} if form == "bit-spins" else None
    with make(sg, g, S0, options=opts, cache="on" if form == "cache-on" else "off") as e:
        e.set_temperatures(np.geomspace(3.0, 0.5, R6))
        e.sweep(10)
        S = e.spins()
        assert not np.array_equal(S, S0)
        check(e, S, planes, 6)
        best = np.stack([e.best(r)[1] for r in range(R6)])
        assert not np.array_equal(best, S)
        check(e, best, planes, 6, which="best", device_map=True)
        check(e, S, planes, 6, which="current", device_map=True, device_out=True)


# ---- 3. every kind of problem: only the spin rows are read ---------------------------------------------------------------
def against_spins(e, rng, n_classes=5, models=1):
    S, R = e.spins(), e.R
    assert S.shape == (R, e.n)
    pairs = [(a, b) for a in range(R) for b in range(R)]
    classes = np.stack([rng.randint(-1, n_classes + 1, e.n), np.arange(e.n) % n_classes]).astype(np.int32)
    got = e.class_overlaps(pairs, classes, n_classes)
    assert np.array_equal(got, cor.pair_form(S, pairs, classes, n_classes))
    # map 1 gives every site a class: the counts add up to the distance (ragged: a pair across models, a row of +-1
    # against zero padding, is meaningless, and the two calls need not agree on it)
    same = np.asarray([a * models // R == b * models // R for a, b in pairs])
    assert np.array_equal(got[:, 1].sum(axis=1)[same], e.pair_overlaps(pairs, links=False)[0][same])
    assert got.any()
    return S, classes, got


def test_dense_shared_csr_ragged_groups_and_tsp_engines(sg):
    from spin_glass_anneal_rl_amd import encoders as enc
    rng = np.random.RandomState(30)
    n = 40
    J = np.triu(rng.randint(0, 2, (n, n)) * 2 - 1, 1).astype(np.float32)
    J = J + J.T
    with sg.AnnealEngine(0) as e:
        e.set_dense(J, np.zeros(n, np.float32))
        e.init_replicas(4, seed=1)
        against_spins(e, rng)
    with sg.AnnealEngine(0) as e:
        e.set_dense_shared(J, rng.randint(-2, 3, (2, n)).astype(np.float32))
        e.init_replicas(4, seed=1)
        against_spins(e, rng)  # pairs across the two field vectors too: the rows are all there is
    with sg.AnnealEngine(0) as e:
        e.set_csr(*torus(6, rng), np.zeros(36, np.float32))
        e.init_replicas(4, seed=1)
        against_spins(e, rng)
    with sg.AnnealEngine(0) as e:  # ragged: rows are zero past a model's own sites and never differ there
        e.set_csr_batch([chain(12, rng) + (np.zeros(12, np.float32),), chain(9, rng) + (np.zeros(9, np.float32),)])
        e.init_replicas(4, seed=1)
        S, classes, got = against_spins(e, rng, models=2)
        assert e.n == 12 and not S[2:, 9:].any() and np.all(classes[1, 9:] >= 0)  # the map names the padded sites of model 1
        own = cor.pair_form(S[:, :9], [(2, 3)], classes[:, :9], 5)[0]
        assert np.array_equal(got[2 * 4 + 3], own)  # ... and they count nothing
    with sg.AnnealEngine(0) as e:
        ng, mp, mem, c, h = gc._assignment(6, 6)
        e.set_groups(ng, (mp, mem), c, h)
        e.init_replicas(4, seed=1)
        against_spins(e, rng)
    with sg.AnnealEngine(0) as e:
        xy = rng.rand(6, 2) * 100.0
        d32, A, B, h, _ = enc.tsp_structure(np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1]), 200.0, 120.0,
                                            auto_scale=True)
        e.set_tsp(d32, A, B, h)
        e.init_replicas(4, seed=1)
        against_spins(e, rng)


# ---- 4. the ladder form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ladders,L", [(2, 8), (4, 4)])
def test_ladder_form_sums(sg, n_ladders, L):
    Ls, rounds = 4, 3
    n, Cn, M = Ls ** 3, Ls, 3
    rng = np.random.RandomState(40 + n_ladders)
    g = lattice3d(Ls, rng)
    planes = sg.encoders.lattice_planes((Ls, Ls, Ls))
    dmap = torch.from_numpy(planes).cuda()
    R, P = n_ladders * L, n_ladders // 2
    #            name          (lo, hi)    sum2
    variants = {"both":       ((0, L),     True),
                "sum1-only":  ((0, L),     False),
                "slot-range": ((1, L - 1), True)}
    dev, ref = {}, {}
    for name, ((lo, hi), second) in variants.items():
        dev[name] = (torch.zeros((P, hi - lo, M, Cn), dtype=torch.int64, device="cuda"),
                     torch.zeros((P, hi - lo, M, Cn, Cn), dtype=torch.int64, device="cuda") if second else None)
        ref[name] = (np.zeros((P, hi - lo, M, Cn), np.uint64), np.zeros((P, hi - lo, M, Cn, Cn), np.uint64) if second else None)
    with make(sg, g, random_spins(R, n, rng)) as e:
        e.set_ladder(np.tile(np.geomspace(4.0, 0.8, L), n_ladders), n_ladders)
        for _ in range(rounds):
            e.sweep(2)
            e.exchange()
            sm, S = e.slot_map(), e.spins()
            for name, ((lo, hi), second) in variants.items():
                assert e.accumulate_ladder_class_overlaps(dmap, Cn, dev[name][0], dev[name][1], slot_lo=lo, slot_hi=hi) is None
                cor.accumulate(ref[name][0], ref[name][1], sm, L, S, planes, Cn, slot_lo=lo, slot_hi=hi)
        assert not np.array_equal(sm, np.arange(R))  # the exchanges permuted the slot map
        s1 = dev["both"][0]
        assert e._lib.sga_accumulate_ladder_class_overlaps(e._h, 2, 2, C.c_void_p(dmap.data_ptr()), n, M, Cn, C.c_void_p(s1.data_ptr()),
                                                           None) == 0  # an empty range: a no-op
        torch.cuda.synchronize()
        for name in variants:
            for got, want in zip(dev[name], ref[name]):
                if want is None:
                    assert got is None
                    continue
                assert np.array_equal(got.cpu().numpy().view(np.uint64), want), name
        both1, both2 = ref["both"]
        assert both1.any() and np.array_equal(both1.sum(axis=3)[:, :, 0], both1.sum(axis=3)[:, :, 1])  # every map sums to the distance
        assert np.array_equal(both2, both2.transpose(0, 1, 2, 4, 3))  # D_c D_c' is symmetric


# ---- 5. refusals leave the sums and the outputs untouched --------------------------------------------------------------
def refused(sg, code, fn, *args, **kw):
    with pytest.raises(sg.AnnealingError) as exc:
        fn(*args, **kw)
    assert exc.value.details["code"] == code, str(exc.value)
    return str(exc.value)


def test_invalid_arguments_are_refused(sg):
    N, rng = sg._native, np.random.RandomState(50)
    g = torus(6, rng)
    n, M, Cn = 36, 2, 6
    planes = sg.encoders.lattice_planes((6, 6))
    with make(sg, g, random_spins(6, n, rng)) as e:
        lib, h = e._lib, e._h
        dmap = torch.from_numpy(planes).cuda()
        s1 = torch.full((1, 3, M, Cn), 7, dtype=torch.int64, device="cuda")
        s2 = torch.full((1, 3, M, Cn, Cn), 7, dtype=torch.int64, device="cuda")
        d = torch.full((2, M, Cn), -5, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        cp, p1, p2, dp = (C.c_void_p(t.data_ptr()) for t in (dmap, s1, s2, d))
        acc = lib.sga_accumulate_ladder_class_overlaps
        assert acc(h, 0, 1, cp, n, M, Cn, p1, p2) == N.ERR_INVALID  # no ladder yet
        assert "no ladder" in N.last_error()
        e.set_ladder(np.tile([2.0, 1.0], 3), 3)  # an odd number of ladders
        assert "even" in refused(sg, N.ERR_INVALID, e.accumulate_ladder_class_overlaps, dmap, Cn,
                                 torch.zeros((1, 2, M, Cn), dtype=torch.int64, device="cuda"))
        e.set_ladder(np.tile([2.0, 1.0, 0.5], 2), 2)
        for lo, hi in ((-1, 2), (0, 4), (2, 1), (3, 4)):
            assert acc(h, lo, hi, cp, n, M, Cn, p1, p2) == N.ERR_INVALID
        host1, host2 = np.full((1, 3, M, Cn), 7, np.uint64), np.full((1, 3, M, Cn, Cn), 7, np.uint64)
        hp1, hp2, hmap = (a.ctypes.data_as(C.c_void_p) for a in (host1, host2, planes))
        assert acc(h, 0, 3, cp, n, M, Cn, hp1, None) == N.ERR_INVALID   # a host sum1
        assert acc(h, 0, 3, cp, n, M, Cn, p1, hp2) == N.ERR_INVALID     # a host sum2
        assert acc(h, 0, 3, hmap, n, M, Cn, p1, p2) == N.ERR_INVALID    # a host map in the ladder form
        assert acc(h, 0, 3, None, n, M, Cn, p1, p2) == N.ERR_INVALID
        assert acc(h, 0, 3, cp, n, M, Cn, None, p2) == N.ERR_INVALID
        assert acc(None, 0, 3, cp, n, M, Cn, p1, p2) == N.ERR_INVALID
        assert acc(h, 0, 3, cp, n, 0, Cn, p1, p2) == N.ERR_INVALID      # n_maps = 0
        assert acc(h, 0, 3, cp, n, M, 0, p1, p2) == N.ERR_INVALID       # n_classes = 0
        assert acc(h, 0, 3, cp, n - 1, M, Cn, p1, p2) == N.ERR_INVALID  # ld < n
        assert acc(h, 0, 3, cp, n, 1, cor.MAX_MC + 1, p1, None) == N.ERR_UNSUPPORTED
        s1_4 = torch.full((1, 4, M, Cn), 7, dtype=torch.int64, device="cuda")
        assert "slot range" in refused(sg, N.ERR_INVALID, e.accumulate_ladder_class_overlaps, dmap, Cn, s1_4, slot_hi=4)  # three slots
        torch.cuda.synchronize()
        assert bool((s1_4 == 7).all())
        # the pair form
        for pairs in ([(0, 1), (0, 6)], [(-1, 2), (0, 1)]):  # an index R, an index -1
            refused(sg, N.ERR_INVALID, e.class_overlaps, pairs, dmap, Cn, out=d)
        pr = np.asarray([[0, 1], [2, 3]], np.int32)
        pp = pr.ctypes.data_as(C.c_void_p)
        get = lib.sga_get_class_overlaps
        assert get(h, 0, pp, 2, cp, n, M, Cn, None) == N.ERR_INVALID      # a NULL output
        assert get(h, 0, pp, 2, None, n, M, Cn, dp) == N.ERR_INVALID      # a NULL map
        assert get(h, 2, pp, 2, cp, n, M, Cn, dp) == N.ERR_INVALID        # which outside {0, 1}
        assert get(h, -1, pp, 2, cp, n, M, Cn, dp) == N.ERR_INVALID
        assert get(h, 0, pp, -1, cp, n, M, Cn, dp) == N.ERR_INVALID       # count < 0
        assert get(h, 0, None, 2, cp, n, M, Cn, dp) == N.ERR_INVALID      # a NULL list with count > 0
        assert get(h, 0, pp, 2, cp, n, 0, Cn, dp) == N.ERR_INVALID
        assert get(h, 0, pp, 2, cp, n, M, -1, dp) == N.ERR_INVALID
        assert get(h, 0, pp, 2, cp, n - 1, M, Cn, dp) == N.ERR_INVALID
        assert get(None, 0, pp, 2, cp, n, M, Cn, dp) == N.ERR_INVALID
        assert get(h, 0, None, 0, cp, n, M, Cn, dp) == N.OK  # count == 0: a no-op
        torch.cuda.synchronize()
        assert bool((s1 == 7).all()) and bool((s2 == 7).all()) and np.all(host1 == 7) and np.all(host2 == 7)
        assert bool((d == -5).all())
        # and the calls still work
        e.accumulate_ladder_class_overlaps(dmap, Cn, s1, s2)
        torch.cuda.synchronize()
        want1, want2 = np.full((1, 3, M, Cn), 7, np.uint64), np.full((1, 3, M, Cn, Cn), 7, np.uint64)
        cor.accumulate(want1, want2, e.slot_map(), 3, e.spins(), planes, Cn)
        assert np.array_equal(s1.cpu().numpy().view(np.uint64), want1) and np.array_equal(s2.cpu().numpy().view(np.uint64), want2)
    with make(sg, g, random_spins(4, n, rng), R_global=8, replica0=4) as e:  # a shard: the ladder form needs all replicas
        e.set_ladder(np.tile([2.0, 1.0, 0.5, 0.3], 2), 2)
        s1 = torch.full((1, 4, M, Cn), 7, dtype=torch.int64, device="cuda")
        assert "R_local" in refused(sg, N.ERR_INVALID, e.accumulate_ladder_class_overlaps, torch.from_numpy(planes).cuda(), Cn, s1)
        torch.cuda.synchronize()
        assert bool((s1 == 7).all())
        S = e.spins()
        assert np.array_equal(e.class_overlaps([(0, 3)], planes, Cn), cor.pair_form(S, [(0, 3)], planes, Cn))  # local indices
    with sg.AnnealEngine(0) as e:  # no problem, then no replicas
        pr = np.zeros(2, np.int32)
        dd = np.full((1, M, Cn), -5, np.int32)
        for _ in range(2):
            assert e._lib.sga_get_class_overlaps(e._h, 0, pr.ctypes.data_as(C.c_void_p), 1, planes.ctypes.data_as(C.c_void_p), n, M, Cn,
                                                 dd.ctypes.data_as(C.c_void_p)) == N.ERR_INVALID
            e.set_csr(*g, np.zeros(n, np.float32))
        assert np.all(dd == -5)


# ---- 6. nothing moves --------------------------------------------------------------------------------------------------
def test_a_run_with_the_calls_interleaved_walks_the_same_chain(sg):
    n_ladders, L, n, Cn = 2, 4, 36, 6
    rng = np.random.RandomState(60)
    g = torus(6, rng)
    h = rng.randint(-1, 2, n).astype(np.float32)
    s0 = random_spins(n_ladders * L, n, rng)
    temps = np.tile(np.geomspace(3.0, 0.6, L), n_ladders)
    planes = sg.encoders.lattice_planes((6, 6))
    dmap = torch.from_numpy(planes).cuda()
    s1 = torch.zeros((1, L, 2, Cn), dtype=torch.int64, device="cuda")
    s2 = torch.zeros((1, L, 2, Cn, Cn), dtype=torch.int64, device="cuda")
    pairs = [(0, 7), (3, 3), (5, 1)]
    with make(sg, g, s0, h=h, cache="on") as a, make(sg, g, s0, h=h, cache="on") as b:
        for e in (a, b):
            e.set_ladder(temps, n_ladders)
        for k in range(20):
            a.sweep(1)
            b.sweep(1)
            kernel = b.last_kernel()
            b.class_overlaps(pairs, planes, Cn)
            b.class_overlaps(pairs, dmap, Cn, which="best")
            b.accumulate_ladder_class_overlaps(dmap, Cn, s1, s2)
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
        assert int(s1.sum()) > 0 and int(s2.sum()) > 0


# ---- 7. ParallelTempering ----------------------------------------------------------------------------------------------
def pt_model(sg, g, n):
    J = np.zeros((n, n), np.float32)
    for i in range(n):
        J[i, g[1][g[0][i]:g[0][i + 1]]] = g[2][g[0][i]:g[0][i + 1]]
    m = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=True))
    m.set_couplings_from_matrix(torch.from_numpy(J))
    return m


def test_parallel_tempering_measures_class_overlaps(sg):
    from spin_glass_anneal_rl_amd.gpu_annealer import fresh_seed
    from spin_glass_anneal_rl_amd.spin_dynamics import UpdateRule, rule_code
    Ls, R = 4, 5
    n = Ls ** 3
    g = lattice3d(Ls, np.random.RandomState(70))
    m = pt_model(sg, g, n)
    planes = sg.encoders.lattice_planes((Ls, Ls, Ls))
    cfg = dict(n_replicas=R, n_sweeps=20, temp_min=0.4, temp_max=3.0, exchange_interval=2, record_interval=2, random_seed=321,
               n_copies=2, autotune=False, measure_class_overlaps=True, overlap_classes=planes, measure_after=4, measure_interval=2)
    pt = sg.ParallelTempering(sg.ParallelTemperingConfig(**cfg))
    res = pt.run(m)
    st = pt.class_overlap_statistics
    # exchange rounds behind sweeps 2, 4 ... 18; from sweep 4 on every second one: those behind sweeps 4, 8, 12, 16
    assert st.measurements == 4 and st.sum1.shape == (1, R, 3, Ls) and st.sum2.shape == (1, R, 3, Ls, Ls)
    assert st.sum1.dtype == np.uint64 and np.array_equal(st.class_sizes, np.full((3, Ls), Ls * Ls))
    assert np.array_equal(st.temperatures, np.asarray(pt.temperatures))
    # the same chain by hand, re-accumulated on the host from the slot map and the spins of the measured rounds
    want1, want2 = np.zeros(st.sum1.shape, np.uint64), np.zeros(st.sum2.shape, np.uint64)
    with sg.AnnealEngine(0) as e:
        e.set_field_cache("auto")
        m.load_into(e, storage="auto")
        e.set_update_rule(rule_code(UpdateRule.METROPOLIS))
        e.init_replicas(2 * R, seed=fresh_seed(321))
        e.set_ladder(np.tile(np.asarray(pt.temperatures, np.float64), 2), 2)
        sweep = 0
        while sweep < 20:
            stop = sweep
            while stop < 19 and not pt._event(stop):
                stop += 1
            e.sweep(stop - sweep + 1, site_mode=sg._native.SITE_RANDOM)
            if stop % 2 == 0 and stop > 0:
                e.exchange(count=False)
                if stop in (4, 8, 12, 16):
                    cor.accumulate(want1, want2, e.slot_map(), R, e.spins(), planes, Ls)
            sweep = stop + 1
        assert np.array_equal(e.spins()[e.slot_map()[:R]], pt.final_spins)  # it was the same chain
    assert np.array_equal(st.sum1, want1) and np.array_equal(st.sum2, want2) and want1.any()
    xi = st.correlation_length()
    assert xi.shape == (R,) and st.susceptibility(0.0).shape == (R,) and np.all(st.susceptibility(0.0) >= 0)
    # the measurement moves nothing: the same run without it is the parent's run
    off = sg.ParallelTempering(sg.ParallelTemperingConfig(**dict(cfg, measure_class_overlaps=False)))
    res_off = off.run(m)
    assert off.class_overlap_statistics is None
    assert res.best_energy == res_off.best_energy
    assert np.array_equal(res.best_configuration.numpy(), res_off.best_configuration.numpy())
    assert np.array_equal(pt.final_spins, off.final_spins)
    assert np.array_equal(pt.exchange_accepts, off.exchange_accepts) and np.array_equal(pt.exchange_attempts, off.exchange_attempts)
    assert res.energy_history == res_off.energy_history
    # beside measure_overlaps and the cluster moves: both measure in the same rounds
    both = sg.ParallelTempering(sg.ParallelTemperingConfig(**dict(cfg, measure_overlaps=True, cluster_moves=True)))
    both.run(m)
    assert both.overlap_rounds_measured == both.class_overlap_statistics.measurements == 4
    d_sum = (both.overlap_statistics.hist_q[0] * np.arange(n + 1)).sum(axis=1)  # the distances summed over the rounds
    assert np.array_equal(both.class_overlap_statistics.sum1[0].sum(axis=2), np.repeat(d_sum[:, None], 3, axis=1).astype(np.uint64))
