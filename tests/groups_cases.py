"""Problems and oracle runs shared by tests/test_groups_host.py and tests/test_groups_gpu.py (test infrastructure).

The oracle never learns about groups: every reference is `oracle.Problem(csr=...)` on the couplings MATERIALISED from
the groups, J_ij = sum of coeff[g] over the groups that hold both i and j (i != j).  Weights are small (|coeff| <= 4)
so that a 10 -> 0.1 ladder accepts some proposals and refuses others on every instance."""
import functools

import numpy as np

import oracle

SEED = 5  # (every instance meets the input conditions of tests/test_groups_host.py at this seed)
WINDOW = 128  # updates one wave of sweep_groups_kernel decides per round: 64 Philox blocks


def materialise(n, member_ptr, members, coeff):
    """(rowptr int32, colidx int32, val fp32) of the couplings the groups stand for, both triangles, rows sorted."""
    import scipy.sparse as sp
    rows, cols, vals = [], [], []
    for g in range(len(member_ptr) - 1):
        m = np.asarray(members[member_ptr[g]:member_ptr[g + 1]], np.int64)
        if m.size < 2:
            continue
        a, b = np.nonzero(~np.eye(m.size, dtype=bool))
        rows.append(m[a])
        cols.append(m[b])
        vals.append(np.full(a.size, np.float64(coeff[g])))
    if not rows:
        z = np.zeros(0, np.int32)
        return np.zeros(n + 1, np.int32), z, np.zeros(0, np.float32)
    J = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    J.sum_duplicates()
    J.sort_indices()
    return J.indptr.astype(np.int32), J.indices.astype(np.int32), J.data.astype(np.float32)


def _pack(n, groups, coeff, h):
    rows = [np.asarray(g, np.int32).ravel() for g in groups]
    mp = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    return n, mp, np.concatenate(rows).astype(np.int32), np.asarray(coeff, np.float32), np.asarray(h, np.float32)


def _assignment(a, t):
    from spin_glass_anneal_rl_amd.encoders import assignment_groups
    costs = np.round(np.random.default_rng(1).uniform(0, 4, a * t) * 8) / 8  # (breaks the ties of the bare penalty)
    n, mp, mem, c, h, _ = assignment_groups(a, t, weight=8.0, costs=costs)     # coeff = -4
    return n, mp, mem, c, h


def _scheduling():
    # 6 tasks x 1 agent x 12 slots, durations of 1-3 slots: a site lies in 1 + duration groups, and two starts of
    # different tasks that overlap in two slots are coupled through two capacity groups -- J accumulates
    from spin_glass_anneal_rl_amd.encoders import scheduling_groups
    n, mp, mem, c, h, _ = scheduling_groups([1.0, 2.0, 3.0, 1.0, 2.0, 3.0], 1, 12, 12,
                                            penalty_weights={"assignment": 4.0, "capacity": 2.0})
    return n, mp, mem, c, h


BIG_N = 700


def _big():
    """n = 700: 700 = 5 x 128 + 60 updates per sweep, so the last window is partial, and at 1, 2 or 4 waves per replica
    a sweep is 6, 3 or 2 super-windows (more than one at every geometry the tests run).  One 300-member group (its sum
    ranges over +-300, far beyond the 128 candidates of a window), rows and columns of a 20 x 20 grid behind it with
    another coefficient, a singleton group, site 699 in no group, half-integer fields."""
    n = BIG_N
    grid = 300 + np.arange(400).reshape(20, 20)
    groups = [np.arange(300)] + [grid[i] for i in range(20)] + [grid[:, j] for j in range(20)]
    groups[20] = groups[20][:-1]          # (site 699 leaves its row ...
    groups[40] = groups[40][:-1]          #  ... and its column: in no group)
    groups.append(np.asarray([650]))      # a singleton
    coeff = [-2.0] + [-4.0] * 40 + [-12.0]
    rng = np.random.default_rng(5)
    h = rng.integers(-4, 5, n) / 2.0
    return _pack(n, groups, coeff, h)


def _one_group():
    return _pack(3, [[0, 1, 2]], [-1.0], [0.5, -1.0, 0.25])


BUILDERS = {
    "one_group_n3": _one_group,
    "assignment_5x7": lambda: _assignment(5, 7),
    "assignment_8x8": lambda: _assignment(8, 8),
    "assignment_13x23": lambda: _assignment(13, 23),
    "scheduling_6x1x12": _scheduling,
    "big_n700": _big,
}
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def problem(name):
    """(n, member_ptr, members, coeff, h, csr) -- csr the materialised couplings."""
    n, mp, mem, c, h = BUILDERS[name]()
    return n, mp, mem, c, h, materialise(n, mp, mem, c)


def ladder(R, hot=10.0, cold=0.1):
    return np.geomspace(hot, cold, R) if R > 1 else np.asarray([1.0])


R_MAIN, SWEEPS = 4, 4


def run_protocol(e, temps, seed=SEED, exchange=True):
    """2 sweeps, one exchange round, 2 sweeps on an engine-like object; everything the tests compare."""
    e.init_replicas(len(temps), seed=seed)
    e.set_ladder(temps, 1)
    t0 = e.sweep(2, energy_trace=True)["energy_trace"]
    swapped = e.exchange() if exchange else 0
    t1 = e.sweep(2, energy_trace=True)["energy_trace"]
    best = [e.best(r) for r in range(len(temps))]
    return dict(spins=e.spins(), energies=e.energies(), trace=np.concatenate([t0, t1]), accepted=e.stats()[0],
                swapped=swapped, slot_map=e.slot_map(), best_energy=np.asarray([b[0] for b in best]),
                best_spins=np.stack([b[1] for b in best]))


@functools.lru_cache(maxsize=None)
def oracle_run(name, R=R_MAIN):
    from oracle_engine import OracleEngine
    n, mp, mem, c, h, csr = problem(name)
    return run_protocol(OracleEngine(h=h, csr=csr), ladder(R))


@functools.lru_cache(maxsize=None)
def oracle_traced(name, R=R_MAIN, n_sweeps=SWEEPS, **kw):
    """Per-update accept / dE traces of `n_sweeps` production sweeps (no exchange) and the proposed sites."""
    n, mp, mem, c, h, csr = problem(name)
    prob = oracle.Problem(h=h, csr=csr)
    s = oracle.init_spins(n, R, SEED)
    out = oracle.sweeps(prob, s, ladder(R), n_sweeps, seed=SEED, trace=True, **kw)
    sites = np.asarray([[[oracle.stream_site(SEED, r, k, t, n) for t in range(n)] for k in range(n_sweeps)]
                        for r in range(R)]).reshape(R, n_sweeps * n)
    return dict(accept=out["accept_trace"], dE=out["dE_trace"], sites=sites, spins=s, energy=out["energy"],
                n_accepted=out["n_accepted"])


def site_groups(name):
    n, mp, mem, c, h, _ = problem(name)
    out = [set() for _ in range(n)]
    for g in range(len(mp) - 1):
        for i in mem[mp[g]:mp[g + 1]]:
            out[int(i)].add(g)
    return out
