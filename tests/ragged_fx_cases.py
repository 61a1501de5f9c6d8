"""Shared problems of the ragged fixed-point cached-field tests (options "ragged_field_cache" and "clf_fixed_point"
together): three batches of sparse models the int16 form refuses, their per-model ladders and the CPU oracle run on EACH
MODEL ALONE with replica0 = m * k (ragged_clf_cases.OracleBatch) -- the reference every test compares against.  The
smallest shapes at which the ragged fixed-point kernel can go wrong:

  batch A (int32 fields, four waves per replica, one entry per thread)
    0  n = 3     complete, J on a 2^-3 grid           smaller than one window, smaller than a wave
    1  n = 37    p = 0.3, J on a 2^-9 grid, h = 0.3 r  odd n; the finest grid: batch-wide k = 9 > k_m of every other model
    2  n = 100   p = 0.9, integer J, h = 0.3 r         rows longer than a wave; the integer model the int16 form refuses
    3  n = 257   p = 0.05, J on a 2^-6 grid           n = 1 mod 32
    4  n = 700   mean degree 12, J on a 2^-6 grid     512 + 188 updates: the second super-window partial
  batch B (int64 fields)
    A's models 0 and 1, a 12-city TSP (encoders.tsp_csr, distances rounded to 2^-10), and n = 40 with one coupling pair
    of 2^22 beside values on a 2^-10 grid: 2^k max_i sum_j |J_ij| >= 2^31
  batch C (a row of more than 512 entries: eight waves per replica, two entries per thread)
    A's models 0 and 1, then n = 1500 with p = 0.4 on a 2^-4 grid (rows of ~ 600 entries)

("h = 0.3 r": 0.3 times one of -2, -1, 1, 2 -- no multiple of 1/2.)  k = 3 replicas per model, ladders as
ragged_clf_cases.model_ladder; the model with the 2^22 pair takes the typical field of its SMALL couplings (the pair
freezes after its first move; the other 38 sites are what walks).  Nothing here needs a GPU.  The cached problems and
references are shared: callers must not write into them."""
import functools

import numpy as np

import ragged_clf_cases as rc

K, SEED, N_SWEEPS = rc.K, rc.SEED, rc.N_SWEEPS


def grid_sparse(n, density, seed, grid_bits, jmax=2.0):
    """Symmetric sparse J with a zero diagonal, values m 2^-grid_bits with 0 < |m 2^-grid_bits| <= jmax, at least one m
    odd (the model's own k is grid_bits exactly), as CSR with strictly sorted rows."""
    rng = np.random.RandomState(seed)
    mask = np.triu(rng.rand(n, n) < density, 1)
    top = int(jmax * 2 ** grid_bits)
    m = rng.randint(1, top + 1, (n, n)) * (rng.randint(0, 2, (n, n)) * 2 - 1)
    i, j = np.argwhere(mask)[0]
    m[i, j] |= 1
    J = np.where(mask, m, 0).astype(np.float64) * 2.0 ** -grid_bits
    J = (J + J.T).astype(np.float32)
    assert np.array_equal(J.astype(np.float64) * 2.0 ** grid_bits, np.rint(J.astype(np.float64) * 2.0 ** grid_bits))
    return rc.dense_to_csr(J)


def lowest_bit_exponent(val):
    """minus the exponent of the lowest set bit of any value: the k of the fixed-point form"""
    v = np.abs(val[val != 0].astype(np.float64))
    k = -1100
    for x in np.unique(v):
        m, e = np.frexp(x)
        q = int(np.ldexp(m, 53))
        k = max(k, -(int(e) - 53 + ((q & -q).bit_length() - 1)))
    return k


def odd_fields(n, seed):
    """h = 0.3 r, r one of -2, -1, 1, 2: fp32 values that are no multiple of 1/2 (and never zero: beside integer J no site
    has a zero field, so a cold replica has no free flips)"""
    r = np.random.RandomState(seed).choice(np.asarray([-2, -1, 1, 2]), n)
    return (r * np.float32(0.3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _model(name):
    if name == "a0":
        return grid_sparse(3, 1.0, 500, 3) + (np.asarray([1.0, -1.0, 1.0], np.float32),)
    if name == "a1":
        return grid_sparse(37, 0.3, 501, 9) + (odd_fields(37, 601),)
    if name == "a2":
        return rc.sym_sparse(100, 0.9, 502) + (odd_fields(100, 602),)
    if name == "a3":
        return grid_sparse(257, 0.05, 503, 6) + (rc.fields(257, 603),)
    if name == "a4":
        return grid_sparse(700, 12.0 / 699.0, 504, 6) + (rc.fields(700, 604),)
    if name == "long":
        return grid_sparse(1500, 0.4, 505, 4) + (rc.fields(1500, 605),)
    if name == "tsp":
        from spin_glass_anneal_rl_amd import encoders
        rng = np.random.RandomState(506)
        xy = rng.rand(12, 2)
        d = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)) * 64.0
        d = np.rint(d * 1024.0) / 1024.0  # distances on a 2^-10 grid
        rowptr, colidx, val, h, _ = encoders.tsp_csr(d)
        return (rowptr.numpy().astype(np.int32), colidx.numpy().astype(np.int32), val.numpy().astype(np.float32),
                h.numpy().astype(np.float32))
    assert name == "wide"
    rp, ci, v = grid_sparse(40, 0.2, 507, 10)
    J = np.zeros((40, 40), np.float32)
    for r in range(40):
        J[r, ci[rp[r]:rp[r + 1]]] = v[rp[r]:rp[r + 1]]
    J[0, 1] = J[1, 0] = np.float32(2.0 ** 22)
    return rc.dense_to_csr(J) + (rc.fields(40, 607),)


_BATCHES = {"A": ("a0", "a1", "a2", "a3", "a4"), "B": ("a0", "a1", "tsp", "wide"), "C": ("a0", "a1", "long")}


@functools.lru_cache(maxsize=None)
def batch(name):
    """The models of batch "A" | "B" | "C" as a tuple of (rowptr, colidx, val, h)."""
    return tuple(_model(m) for m in _BATCHES[name])


def batch_k(probs):
    """the batch-wide k: the finest grid any model needs"""
    return max(lowest_bit_exponent(p[2]) for p in probs)


def batch_bound(probs):
    """2^k max_i sum_j |J_ij| over all rows of the batch: below 2^31 int32 fields, else int64"""
    k = batch_k(probs)
    worst = max(float(np.add.reduceat(np.abs(p[2].astype(np.float64)), p[0][:-1][np.diff(p[0]) > 0]).max()) for p in probs)
    return worst * 2.0 ** k


def model_ladder(p, k=K, hot=6.0, cold=0.25):
    """ragged_clf_cases.model_ladder; a model with a coupling of 2^20 or more: in units of the field of the others"""
    big = np.abs(p[2]) >= 2.0 ** 20
    if big.any():
        p = (p[0], p[1], np.where(big, 0, p[2]).astype(np.float32), p[3])
    return rc.model_ladder(p, k, hot=hot, cold=cold)


def ladders(probs, k=K, **kw):
    return np.concatenate([model_ladder(p, k, **kw) for p in probs])


@functools.lru_cache(maxsize=None)
def reference(name, rule=None, arith=None):
    """Batch `name` after N_SWEEPS sweeps on its ladders: (OracleBatch, energy trace).  Shared: read only."""
    probs = batch(name)
    ob = rc.OracleBatch(probs, ladders(probs))
    kw = {}
    if rule is not None:
        kw["rule"] = rule
    if arith is not None:
        kw["arith"] = arith
    trace = ob.sweep(N_SWEEPS, **kw)
    return ob, trace


def check_acceptance(name):
    """As ragged_clf_cases.check_acceptance: over the reference run every model with n >= 37 accepts some proposals and
    rejects some; the hot replica accepts more than half, the cold one fewer than the hot one and less than half.
    Returns the per-replica acceptance."""
    ob, _ = reference(name)
    out = []
    for m, n in enumerate(ob.sizes):
        rate = ob.n_accepted[m] / float(N_SWEEPS * n)
        out.append(rate)
        if n < 37:
            continue
        assert np.all(rate > 0.0) and np.all(rate < 1.0), (name, m, rate)
        assert rate[0] > 0.5 and rate[-1] < rate[0] and rate[-1] < 0.5, (name, m, rate)
    return out
