"""Every sweep form's random-stream coordinates against the oracle: the GLOBAL replica id (shards with replica0 != 0, a
shard at the far end of 65536 replicas), the sweep counter (from a non-zero start, across the sign bit and across the
wrap at 2^32, through a checkpoint and an autotune) and all 64 bits of the seed -- and the same for the other streams
(initial spins, exchange rounds, pair lists, the operator exchange).

The forms come from tests/stream_forms.py; every case asserts the form's own predicate on last_kernel() / describe(),
so that a form that silently ran something else fails here.  "Equal" is np.array_equal on the energy trace, final
spins, energies, accept counters, per-replica best energies and best spins; the two canonical-sum forms compare their
energies with the oracle at the tolerance of tests/test_temperature_edges_gpu.py and GPU against GPU exactly."""
import numpy as np
import pytest
import torch

import oracle
from oracle_follow import follow
from stream_forms import (BY_NAME, FORMS, MASK32, EngineChain, OracleChain, assert_same, ladder_for, slice_state,
                          temps_for)
from test_temperature_edges_gpu import exchange_engine, oracle_round, pm1

pytestmark = pytest.mark.gpu

SEED = (0x1234ABCD << 32) | 0x0F1E2D3C  # both halves non-zero and different
SEEDS = {"s": SEED, "s+2^32": SEED + 2 ** 32, "halves-swapped": ((SEED & MASK32) << 32) | (SEED >> 32)}
SINGLE = [f for f in FORMS if f.single and f.site_mode == 0]
names = lambda forms: [f.name for f in forms]  # noqa: E731


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def cuts_of(form):
    """Two cuts of the global set into three uneven shards: off every multiple of 32 and off every model boundary."""
    R, M = form.R_global, len(form.build().models)
    a, b = R * 37 // 100, R * 71 // 100
    assert 0 < a < b < R and len({a, b - a, R - b}) == 3
    assert all(c % 32 and c % (R // M) for c in (a, b))
    return [0, a, b, R]


# ----------------------------------------------------------------------------- the global replica id
@pytest.mark.parametrize("name", names(FORMS))
def test_three_uneven_shards_equal_one_engine_and_the_oracle(sg, name):
    form = BY_NAME[name]
    b, R = form.build(), form.R_global
    temps, edges = temps_for(b, R), cuts_of(form)
    with EngineChain(sg, form, R, 0, R, SEED, temps) as one:
        whole = one.run(form.plan)
    for lo, hi in zip(edges[:-1], edges[1:]):
        with EngineChain(sg, form, R, lo, hi - lo, SEED, temps[lo:hi]) as shard:
            got = shard.run(form.plan)
        assert_same(got, slice_state(whole, lo, hi), True, (name, "one engine", lo, hi))
        ref = OracleChain(form, R, lo, hi - lo, SEED, temps[lo:hi])
        for ns in form.plan:
            ref.sweep(ns)
        assert_same(got, ref.state(), form.exact, (name, "oracle", lo, hi))


@pytest.mark.parametrize("name", names(SINGLE))
def test_sharded_ladder_with_exchanges_equals_the_one_engine_ladder(sg, name):
    """Exchange rounds on all-gathered energies move temperatures across the shard borders: the per-temperature accept
    tables of the cached-field forms and AUTO's per-replica routing then work with replica0 != 0."""
    form = BY_NAME[name]
    b, world, R_local = form.build(), 3, 8
    R = world * R_local
    # hot -> cold, cold -> hot, hot -> cold: every shard holds hot and cold slots, and the slots on either side of a
    # shard border carry one temperature, so that every attempt there swaps
    rung = ladder_for(b, R_local)
    slot_temps = np.concatenate([rung if k % 2 == 0 else rung[::-1] for k in range(world)])
    plan = form.plan * 3

    def run(n_engines):
        chains = [EngineChain(sg, form, R, 0, R // n_engines, SEED, init=False) for _ in range(n_engines)]
        try:
            group = sg.LocalShardedTempering([c.e for c in chains], R // n_engines, seed=SEED, slot_temps=slot_temps)
            swaps, maps = [], []
            for i, ns in enumerate(plan):
                group.sweep(ns)
                for c in chains:
                    c.note(last=i + 1 == len(plan))
                swaps.append(group.exchange())
                maps.append(chains[0].e.slot_map())
            states = [c.state() for c in chains]
            merged = {k: [x for s in states for x in s[k]] for k in ("spins", "best_s")}
            merged.update({k: np.concatenate([s[k] for s in states]) for k in ("acc", "energy", "best_e")})
            merged["trace"] = np.concatenate([c.e.temperatures() for c in chains])[None, :]  # (who holds which slot)
            return merged, swaps, np.stack(maps), chains[0].e.exchange_stats()
        finally:
            for c in chains:
                c.e.close()

    one, many = run(1), run(world)
    assert_same(many[0], one[0], True, name)
    assert many[1] == one[1] and np.array_equal(many[2], one[2]), name
    assert all(np.array_equal(x, y) for x, y in zip(many[3], one[3])), name
    # (the slot maps after every round: a replica that crossed a border may have come back by the end)
    assert np.any(one[2] // R_local != np.arange(R)[None, :] // R_local), (name, "no replica crossed a shard border", one[2])


@pytest.mark.parametrize("name", ["row-shared-W256-planes", "clfb-several-accepts", "csr-upd4"])
def test_the_last_shard_of_65536_replicas(sg, name):
    """The last rank's shard of an eight-rank ladder of 8192 replicas per rank, followed on its first, a middle and its
    last replica."""
    form = BY_NAME[name]
    b, R_global, R_local = form.build(), 65536, 40
    g0 = R_global - R_local
    temps = temps_for(b, R_global)
    with EngineChain(sg, form, R_global, g0, R_local, SEED, temps[g0:]) as shard:
        got = shard.run(form.plan)
    prob = b.models[0]
    ref = follow(prob, prob.n, SEED, temps, [g0, g0 + R_local // 2, R_global - 1], sum(form.plan))
    for g, (trace, spins, acc) in ref.items():
        r = g - g0
        assert np.array_equal(got["trace"][:, r], trace), (name, g)
        assert np.array_equal(got["spins"][r], spins) and got["acc"][r] == acc, (name, g)


# ----------------------------------------------------------------------------- the sweep counter
COUNTER_PLAN = (1, 3, 40)  # the 40 in one call: AUTO's 16-sweep pieces and sweeps_per_launch splits advance sweep0


@pytest.mark.parametrize("c0", [2 ** 31 - 2, 2 ** 32 - 2], ids=["sign-bit", "wrap"])
@pytest.mark.parametrize("name", names(FORMS))
def test_counter_from_a_high_start_across_the_sign_bit_and_the_wrap(sg, name, c0):
    form = BY_NAME[name]
    b, R = form.build(), form.R_small
    temps = temps_for(b, R)
    ref = OracleChain(form, R, 0, R, SEED, temps, c0=c0)
    for ns in COUNTER_PLAN:
        ref.sweep(ns)
    with EngineChain(sg, form, R, 0, R, SEED, temps, c0=c0) as run:
        assert run.e.counters() == (c0, 0)
        run.sweep(COUNTER_PLAN[0], last=False)
        blob, first = run.e.export_state(), run.traces[0]
        for i, ns in enumerate(COUNTER_PLAN[1:]):
            run.sweep(ns, last=i == 1)
        assert run.e.counters() == ((c0 + sum(COUNTER_PLAN)) & MASK32, 0), "the counter wraps at 2^32"
        got = run.state()
    assert_same(got, ref.state(), form.exact, (name, c0, "oracle"))
    if c0 == 2 ** 32 - 2:  # a checkpoint from before the wrap, continued by a fresh engine
        with EngineChain(sg, form, R, 0, R, SEED, temps) as fresh:
            fresh.e.import_state(blob)
            assert fresh.e.counters() == (2 ** 32 - 1, 0)
            fresh.traces.append(first)
            for i, ns in enumerate(COUNTER_PLAN[1:]):
                fresh.sweep(ns, last=i == 1)
            assert fresh.e.counters() == (sum(COUNTER_PLAN) - 2, 0)
            assert_same(fresh.state(), got, True, (name, "resumed"))


@pytest.mark.parametrize("name", ["row-shared-W256-planes", "csr-upd4", "dense-f32-look1"])
def test_autotune_in_mid_run_at_a_high_counter_inside_a_shard(sg, name):
    form = BY_NAME[name]
    b, R_global, g0, R, c0 = form.build(), 100, 37, 34, 2 ** 32 - 3
    temps = temps_for(b, R_global)[g0:g0 + R]
    ref = OracleChain(form, R_global, g0, R, SEED, temps, c0=c0)
    ref.sweep(2)
    ref.sweep(4)
    with EngineChain(sg, form, R_global, g0, R, SEED, temps, c0=c0) as run:
        run.sweep(2)
        before = run.state()
        run.e.autotune()
        assert run.e.counters() == (c0 + 2, 0)
        assert_same(run.state(), before, True, (name, "state across autotune"))
        run.traces.append(run.e.sweep(4, energy_trace=True)["energy_trace"])  # (whatever form the autotuner kept)
        assert run.e.counters() == (3, 0)
        assert_same(run.state(), ref.state(), form.exact, (name, "oracle"))


# ----------------------------------------------------------------------------- the seed
@pytest.mark.parametrize("name", names(FORMS))
def test_all_64_seed_bits_key_the_sweeps(sg, name):
    form = BY_NAME[name]
    b, R = form.build(), form.R_small
    temps = temps_for(b, R)
    runs = {}
    for tag, seed in SEEDS.items():
        with EngineChain(sg, form, R, 0, R, seed, temps) as run:
            runs[tag] = run.run(form.plan)
        ref = OracleChain(form, R, 0, R, seed, temps)
        for ns in form.plan:
            ref.sweep(ns)
        assert_same(runs[tag], ref.state(), form.exact, (name, tag))
    tags = list(SEEDS)
    for i, x in enumerate(tags):
        for y in tags[i + 1:]:
            assert not np.array_equal(runs[x]["acc"], runs[y]["acc"]), (name, x, y, "accept counters")
            assert not all(np.array_equal(p, q) for p, q in zip(runs[x]["spins"], runs[y]["spins"])), (name, x, y)


@pytest.mark.parametrize("name", ["dense-i8-look1", "clfb-several-accepts", "row-shared-W256-planes", "csr-upd8",
                                  "tsp-8-updates", "wolff-csr", "dense-batch-cached", "ragged-csr-batch"])
def test_set_seed_in_mid_run_keys_later_sweeps_and_keeps_the_counters(sg, name):
    """include/sga.h: "Philox key of all later draws (sweeps, exchanges); the counters are unchanged"."""
    form = BY_NAME[name]
    b, R, c0 = form.build(), form.R_small, 1000
    temps = temps_for(b, R)
    ref = OracleChain(form, R, 0, R, SEEDS["s"], temps, c0=c0)
    with EngineChain(sg, form, R, 0, R, SEEDS["s"], temps, c0=c0) as run:
        for seed in SEEDS.values():
            run.e.set_seed(seed)
            ref.set_seed(seed)
            done = run.e.counters()
            run.sweep(3)
            ref.sweep(3)
            assert run.e.counters() == (done[0] + 3, 0)
        assert_same(run.state(), ref.state(), form.exact, name)


# ----------------------------------------------------------------------------- the other streams
@pytest.mark.parametrize("tag", list(SEEDS))
@pytest.mark.parametrize("name", ["dense-f32-look1", "csr-upd0", "tsp-one-update", "dense-batch-rows", "ragged-csr-batch"])
def test_initial_spins_of_a_shard(sg, name, tag):
    form = BY_NAME[name]
    R_global = form.R_global
    lo, hi = cuts_of(form)[1:3]
    with EngineChain(sg, form, R_global, lo, hi - lo, SEEDS[tag]) as shard:
        got = shard.state()
    ref = OracleChain(form, R_global, lo, hi - lo, SEEDS[tag], np.ones(hi - lo)).state()
    assert all(np.array_equal(x, y) for x, y in zip(got["spins"], ref["spins"])), (name, tag)
    assert np.array_equal(got["energy"], ref["energy"]), (name, tag)


def _exchange_problem(R, n=48):
    """Replicas at a handful of different energies, so that rounds both accept and reject."""
    J = pm1(n, 21)
    return J, oracle.init_spins(n, R, 5)


@pytest.mark.parametrize("n_ladders", [1, 3])
def test_exchange_rounds_draw_from_all_64_seed_bits(sg, n_ladders):
    L = 8
    R = L * n_ladders
    J, spins = _exchange_problem(R)
    temps = np.tile(np.geomspace(4.0, 0.5, L), n_ladders)
    seen = {}
    for tag, seed in SEEDS.items():
        e = exchange_engine(sg, J, R, seed, temps, n_ladders)
        try:
            for r in range(R):
                e.set_spins(r, spins[r])
            e.set_counters(7, 2 ** 32 - 3)  # the round counter wraps like the sweep counter
            slot, att, acc, log = np.arange(R, dtype=np.int32), np.zeros(R, np.int64), np.zeros(R, np.int64), []
            for rnd in range(6):
                want = oracle_round(temps, e.energies(), slot, L, n_ladders, seed, (2 ** 32 - 3 + rnd) & MASK32, att, acc)
                assert e.exchange() == want, (tag, rnd)
                assert np.array_equal(e.slot_map(), slot), (tag, rnd)
                log.append(slot.copy())
            assert e.counters() == (7, 3)
            a2, c2 = e.exchange_stats()
            assert np.array_equal(a2, att) and np.array_equal(c2, acc)
            seen[tag] = (np.stack(log), att.copy(), acc.copy())
        finally:
            e.close()
    tags = list(seen)
    for i, x in enumerate(tags):
        for y in tags[i + 1:]:
            assert not all(np.array_equal(p, q) for p, q in zip(seen[x], seen[y])), (x, y)


def test_exchange_pairs_draw_from_all_64_seed_bits(sg):
    R = 8
    J, spins = _exchange_problem(R)
    temps = np.geomspace(4.0, 0.5, R)
    pairs = [(5, 6), (0, 1), (4, 5), (0, 6), (2, 7), (1, 3), (6, 7), (3, 4), (1, 2)]
    seen = {}
    for tag, seed in SEEDS.items():
        e = exchange_engine(sg, J, R, seed, temps, 1)
        try:
            for r in range(R):
                e.set_spins(r, spins[r])
            slot, att, acc, log = np.arange(R, dtype=np.int32), np.zeros(R, np.int64), np.zeros(R, np.int64), []
            for rnd in range(6):
                want = oracle.pt_exchange_pairs(temps, e.energies(), slot, pairs, u=None, seed=seed, round_=rnd,
                                                attempts=att, accepts=acc)
                assert e.exchange_pairs(pairs, u=None) == want, (tag, rnd)
                assert np.array_equal(e.slot_map(), slot), (tag, rnd)
                log.append(slot.copy())
            seen[tag] = np.stack(log)
        finally:
            e.close()
    tags = list(seen)
    assert not any(np.array_equal(seen[x], seen[y]) for i, x in enumerate(tags) for y in tags[i + 1:])


def test_operator_exchange_draws_from_all_64_seed_bits(sg):
    """op_pt_exchange(u=None): pair i of round k takes word 0 of Philox block (i, k, 0, domain 1) under the key
    (seed lo, seed hi), as a 24-bit uniform; the oracle's operator exchange is fed those uniforms from its own Philox."""
    from spin_glass_anneal_rl_amd.engine import op_pt_exchange
    R, n = 24, 32
    temps = np.geomspace(4.0, 0.5, R).astype(np.float32)
    spins0 = oracle.init_spins(n, R, 8)
    # energies rising along the ladder by 0.7 / (beta[i + 1] - beta[i]): every decision is a coin of p = 0.5 or less,
    # so that it is the uniforms that decide
    energies0 = np.concatenate([[0.0], np.cumsum(0.7 / np.diff(1.0 / temps.astype(np.float64)))]).astype(np.float32)
    seen = {}
    for tag, seed in SEEDS.items():
        log = []
        for rnd in (0, 5, 2 ** 32 - 1):
            u = np.asarray([np.float32(oracle.philox([i, rnd, 0, 1], [seed & MASK32, seed >> 32])[0] >> 8) * np.float32(2.0 ** -24)
                            for i in range(R - 1)], np.float32)
            s_ref, e_ref = spins0.copy(), energies0.copy()
            want = oracle.pt_exchange_operator(s_ref, e_ref, temps, u)
            sp = torch.from_numpy(spins0.astype(np.float32)).cuda()
            en = torch.from_numpy(energies0.copy()).cuda()
            got = op_pt_exchange(0, sp, en, torch.from_numpy(temps).cuda(), u=None, seed=seed, round_=rnd)
            assert got == want, (tag, rnd)
            assert np.array_equal(sp.cpu().numpy().astype(np.int8), s_ref) and np.array_equal(en.cpu().numpy(), e_ref)
            log.append(e_ref)
        seen[tag] = np.stack(log)
    tags = list(seen)
    assert not any(np.array_equal(seen[x], seen[y]) for i, x in enumerate(tags) for y in tags[i + 1:])


def test_set_seed_in_mid_run_keys_later_exchange_rounds(sg):
    L, n_ladders = 8, 2
    R = L * n_ladders
    J, spins = _exchange_problem(R)
    temps = np.tile(np.geomspace(4.0, 0.5, L), n_ladders)
    e = exchange_engine(sg, J, R, SEEDS["s"], temps, n_ladders)
    try:
        for r in range(R):
            e.set_spins(r, spins[r])
        slot, att, acc = np.arange(R, dtype=np.int32), np.zeros(R, np.int64), np.zeros(R, np.int64)
        rnd = 0
        for seed in SEEDS.values():
            e.set_seed(seed)
            for _ in range(3):
                assert e.counters() == (0, rnd)
                assert e.exchange() == oracle_round(temps, e.energies(), slot, L, n_ladders, seed, rnd, att, acc), (seed, rnd)
                assert np.array_equal(e.slot_map(), slot), (seed, rnd)
                rnd += 1
    finally:
        e.close()
