"""An independent float64 reference of the two canonical row-sum orders of DESIGN.md 2 ("Tolerance statement"), a set
of decoy orders that model real kernel mistakes, and the order-sensitive problems that make the order visible.

Written from the prose of DESIGN.md and include/sga.h, not from oracle/sg_oracle.c or the kernels:

  dense   the row is cut into super-chunks of 1024 elements, a super-chunk into four chunks of 256.  Lane l of 64 adds
          its sixteen products from +0 -- chunk 0..3, elements 4l .. 4l+3 of each, in that order --, the 64 lane sums
          are folded by an adjacent-pairs tree (l += l+1, then l += l+2, ...), the super-chunk sums are added in order.
  CSR     entry e of the row (storage order, duplicates are entries of their own) belongs to lane e % 64 of virtual
          wave (e / 64) % 8; a lane adds its entries in storage order, each virtual wave folds its 64 lanes by the same
          tree, the 8 wave sums are added in order.

Products J * s are exact in fp32; every addition is an fp64 addition; the sum is rounded to fp32 once.

Every function takes the products `P` as a float64 array [..., length] and works on the last axis, so that many
proposals are summed at once.  Positions past the end of a row hold +0.0, which no sum notices.

The problems ("How the order is pinned"): sites are probes or ballast.  Ballast sites come in pairs
(b, b') that hold equal spins; a probe row carries J[i,b] = a, J[i,b'] = -a with a = (full 24-bit mantissa) * 2^k,
k in 30 .. 43.  The big products cancel exactly in pairs, but a partial sum that holds a 2^40-sized term rounds every
O(1) term added to it, so the fp32 value of the row sum depends on the order of the additions.  The ballast must never
flip: replayed runs propose probe sites only, Philox runs pin each ballast site with a field h_b = s_b 2^m.
"""
import numpy as np

K_LO, K_HI = 30, 43  # binary exponents of the ballast couplings


# ---------------------------------------------------------------------------------------------------------------
# sums over the last axis of a float64 array of products
# ---------------------------------------------------------------------------------------------------------------
def _pad(P, multiple):
    P = np.asarray(P, np.float64)
    n = P.shape[-1]
    m = max(multiple, -(-n // multiple) * multiple)
    if m == n:
        return P
    out = np.zeros(P.shape[:-1] + (m,), np.float64)
    out[..., :n] = P
    return out


def _seq(terms):
    """terms [..., k]: ((t0 + t1) + t2) + ... from the first term."""
    return np.add.accumulate(terms, axis=-1)[..., -1]


def tree_adjacent(lanes):
    """[..., 64] -> [...]: l += l + 1 for even l, then l += l + 2 for l % 4 == 0, ... (adjacent pairs first)."""
    v = lanes
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def tree_far(lanes):
    """The decoy tree: l += l + 32 for l < 32 first, then l += l + 16 for l < 16, ..."""
    v = lanes
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


def _dense_lanes(P, k_major=False):
    """[..., n] -> lane sums [..., C, 64] of the C super-chunks."""
    Q = _pad(P, 1024)
    Q = Q.reshape(Q.shape[:-1] + (-1, 4, 64, 4))  # [..., super-chunk, chunk, lane, element]
    Q = np.moveaxis(Q, -2, -3)                     # [..., super-chunk, lane, chunk, element]
    if k_major:
        Q = np.swapaxes(Q, -1, -2)
    return _seq(Q.reshape(Q.shape[:-2] + (16,)))   # starts from the first product: 0 + p0 is p0


def dense_sum64(P, order="canonical"):
    """The fp64 row sum of the products P [..., n] in the canonical dense order, or in one of the decoy orders."""
    P = np.asarray(P, np.float64)
    if order == "left-to-right":
        return _seq(P)
    lanes = _dense_lanes(P, k_major=(order == "k-major"))
    chunks = (tree_far if order == "far-tree" else tree_adjacent)(lanes)  # [..., C]
    if order in ("canonical", "k-major", "far-tree"):
        return _seq(chunks)
    if order in ("by-wave-2", "by-wave-3"):  # each of W waves adds the super-chunks it owns, then the waves are added
        W = int(order[-1])
        waves = [_seq(chunks[..., w::W]) for w in range(W) if chunks[..., w::W].shape[-1]]
        return _seq(np.stack(waves, axis=-1))
    raise ValueError(order)


def _csr_passes(P, span):
    Q = _pad(P, span)
    return Q.reshape(Q.shape[:-1] + (-1, span // 64, 64))  # [..., pass, virtual wave, lane]


def csr_sum64(P, order="canonical"):
    """The fp64 row sum of the products P [..., entries] (storage order) in the canonical CSR order or a decoy."""
    P = np.asarray(P, np.float64)
    if order == "left-to-right":
        return _seq(P)
    if order == "fold-per-pass":  # every pass over the row folded on its own, the folded passes added per wave
        Q = _csr_passes(P, 512)
        return _seq(_seq(np.moveaxis(tree_adjacent(Q), -2, -1)))
    Q = _csr_passes(P, 256 if order == "4-waves" else 512)
    lanes = _seq(np.moveaxis(Q, -3, -1))           # [..., virtual wave, lane]: a lane's entries in storage order
    if order in ("canonical", "4-waves"):
        return _seq(tree_adjacent(lanes))
    if order == "far-tree":
        return _seq(tree_far(lanes))
    raise ValueError(order)


DENSE_DECOYS = ("left-to-right", "k-major", "far-tree", "by-wave-2", "by-wave-3")
CSR_DECOYS = ("left-to-right", "far-tree", "4-waves", "fold-per-pass")


def dense_decoys(n):
    """The decoys that change an addition for a row of n elements, and why the others do not."""
    chunks = -(-n // 1024)
    out = {"left-to-right": None, "k-major": None, "far-tree": None,
           "by-wave-2": None if chunks >= 3 else "fewer than three super-chunks: two waves add them in order",
           "by-wave-3": None if chunks >= 4 else "fewer than four super-chunks: three waves add them in order"}
    return out


def csr_decoys(longest_row):
    out = {"left-to-right": None, "far-tree": None,
           "4-waves": None if longest_row > 256 else "rows of at most 256 entries: a lane holds one entry either way",
           "fold-per-pass": None if longest_row > 512 else "rows of at most 512 entries: one pass over the row"}
    return out


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def products(vals, spins):
    """fp32 products J * s (exact) as float64."""
    return (np.asarray(vals, np.float32) * np.asarray(spins).astype(np.float32)).astype(np.float64)


def dense_row_sum(row, s, order="canonical"):
    """fp32(sum_j row_j s_j) in the canonical dense order."""
    return f32(dense_sum64(products(row, s), order))


def csr_row_sum(vals, cols, s, order="canonical"):
    """fp32(sum_e vals_e s[cols_e]) over the row's entries in storage order, canonical CSR order."""
    return f32(csr_sum64(products(vals, np.asarray(s)[..., np.asarray(cols, np.int64)]), order))


# ---------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------
def _big(rng, size):
    """+-(1.f with all 24 mantissa bits in use) * 2^k, k in K_LO .. K_HI."""
    mant = 1.0 + (rng.randint(0, 1 << 22, size) * 2 + 1) / float(1 << 23)
    return (rng.choice([-1.0, 1.0], size) * mant * 2.0 ** rng.randint(K_LO, K_HI + 1, size)).astype(np.float32)


class Problem:
    """Couplings (dense J or CSR), fields, and who is what.  `ballast_spin[site]` is the spin every replica gives a
    ballast site (0 for probes); with `pinned` the fields hold the ballast there under any finite temperature."""

    def __init__(self, name, n, h, probes, ballast_spin, J=None, csr=None, pinned=False):
        self.name, self.n, self.h, self.J, self.csr, self.pinned = name, n, h, J, csr, pinned
        self.probes, self.ballast_spin = probes, ballast_spin
        self.ballast = np.nonzero(ballast_spin)[0]
        if csr is not None:
            rp = np.asarray(csr[0], np.int64)
            self.row_len = np.diff(rp)
            L = max(1, int(self.row_len.max()))
            self.cols_pad = np.zeros((n, L), np.int64)
            self.vals_pad = np.zeros((n, L), np.float32)
            for i in range(n):
                self.cols_pad[i, :self.row_len[i]] = csr[1][rp[i]:rp[i + 1]]
                self.vals_pad[i, :self.row_len[i]] = csr[2][rp[i]:rp[i + 1]]

    def oracle_problem(self):
        import oracle
        return oracle.Problem(J=self.J, h=self.h) if self.J is not None else oracle.Problem(csr=self.csr, h=self.h)

    def s0(self, R, seed, replica0=0):
        """Initial spins [R, n]: probes from the Philox stream, ballast pairs as the problem fixes them."""
        import oracle
        s = oracle.init_spins(self.n, R, seed, replica0)
        s[:, self.ballast] = self.ballast_spin[self.ballast]
        return s

    def row_products(self, sites, S):
        """Products of row sites[k] with spins S[k]: float64 [B, n] (dense) or [B, longest row] (CSR)."""
        sites = np.asarray(sites, np.int64)
        S = np.asarray(S)
        if self.J is not None:
            return products(self.J[sites], S)
        return products(self.vals_pad[sites], np.take_along_axis(S, self.cols_pad[sites], axis=1))

    def row_sums(self, sites, S, order="canonical"):
        """fp32 row sums of rows sites[k] at spins S[k], as float64."""
        P = self.row_products(sites, S)
        return f32(dense_sum64(P, order) if self.J is not None else csr_sum64(P, order)).astype(np.float64)

    def decoys(self):
        return dense_decoys(self.n) if self.J is not None else csr_decoys(int(self.row_len[self.probes].max()))

    def probe_scale(self):
        """About the size of a probe's |dE|: twice the root of the number of O(1) couplings in its row."""
        if self.J is not None:
            return 2.0 * float(np.sqrt(len(self.probes)))
        v = np.abs(self.vals_pad[self.probes])
        return 2.0 * float(np.sqrt(max(1.0, np.mean(np.sum((v > 0) & (v < 2.0 ** K_LO), axis=1)))))

    def pin_exponent(self):
        A = np.abs(self.J).astype(np.float64).sum(1) if self.J is not None else \
            np.abs(self.vals_pad).astype(np.float64).sum(1)
        return int(np.ceil(np.log2(max(A.max(), 1.0)))) + 2


def _roles(n, n_pairs, rng):
    perm = rng.permutation(n)                       # probes and ballast scattered over the row
    pairs = perm[:2 * n_pairs].reshape(n_pairs, 2)
    probes = np.sort(perm[2 * n_pairs:])
    bs = np.zeros(n, np.int8)
    bs[pairs[:, 0]] = bs[pairs[:, 1]] = rng.choice([-1, 1], n_pairs).astype(np.int8)
    return probes, pairs, bs


def _pin(prob):
    """h_b = s_b 2^m on the ballast, 2^m above every row's sum |J|: a flip there costs ~2^(m+1)."""
    h = prob.h.copy()
    h[prob.ballast] = prob.ballast_spin[prob.ballast].astype(np.float32) * np.float32(2.0 ** prob.pin_exponent())
    prob.h, prob.pinned = h, True
    return prob


def dense_problem(n, seed, pinned=False, pair_share=0.25):
    """Dense probe / ballast problem: n - 2 p probes with randn couplings among them, p = pair_share n ballast pairs,
    every probe coupled to every pair.  Symmetric, zero diagonal, randn fields on the probes."""
    rng = np.random.RandomState(seed)
    probes, pairs, bs = _roles(n, int(n * pair_share), rng)
    J = np.zeros((n, n), np.float32)
    G = np.triu(rng.randn(len(probes), len(probes)), 1).astype(np.float32)
    J[np.ix_(probes, probes)] = G + G.T
    a = _big(rng, (len(probes), len(pairs)))
    J[np.ix_(probes, pairs[:, 0])] = a
    J[np.ix_(probes, pairs[:, 1])] = -a
    J[np.ix_(pairs[:, 0], probes)] = a.T
    J[np.ix_(pairs[:, 1], probes)] = -a.T
    h = np.zeros(n, np.float32)
    h[probes] = rng.randn(len(probes)).astype(np.float32)
    prob = Problem(f"dense-n{n}" + ("-pinned" if pinned else ""), n, h, probes, bs, J=J)
    return _pin(prob) if pinned else prob


def csr_problem(n_probes, pairs_per_row, small_per_row, seed, pinned=False, sort_rows=False):
    """Sparse probe / ballast problem: every probe row holds `pairs_per_row` ballast pairs and up to `small_per_row`
    randn couplings to other probes, in shuffled storage order (or sorted by column).  The pairs are dealt round
    robin, so that no ballast row is longer than a probe row may be.  Symmetric, zero diagonal."""
    rng = np.random.RandomState(seed)
    longest = 2 * pairs_per_row + small_per_row
    n_pairs = max(pairs_per_row, -(-n_probes * pairs_per_row // longest))
    n = n_probes + 2 * n_pairs
    probes, pairs, bs = _roles(n, n_pairs, rng)
    rows = [dict() for _ in range(n)]
    small = [0] * n
    for i in probes:
        for j in probes[rng.randint(0, n_probes, small_per_row // 2)]:
            if i != j and int(j) not in rows[i] and small[i] < small_per_row and small[j] < small_per_row:
                v = np.float32(rng.randn())
                rows[i][int(j)] = rows[j][int(i)] = v
                small[i] += 1
                small[j] += 1
    for k, i in enumerate(probes):
        for t in range(pairs_per_row):
            a = _big(rng, 1)[0]
            b, b2 = (int(v) for v in pairs[(k * pairs_per_row + t) % n_pairs])
            rows[i][b] = rows[b][int(i)] = a
            rows[i][b2] = rows[b2][int(i)] = -a
    rowptr, cols, vals = [0], [], []
    for i in range(n):
        c = np.asarray(sorted(rows[i]), np.int32)
        if not sort_rows:
            c = c[rng.permutation(len(c))]
        cols.append(c)
        vals.append(np.asarray([rows[i][int(j)] for j in c], np.float32))
        rowptr.append(rowptr[-1] + len(c))
    csr = (np.asarray(rowptr, np.int32), np.concatenate(cols).astype(np.int32), np.concatenate(vals).astype(np.float32))
    h = np.zeros(n, np.float32)
    h[probes] = rng.randn(n_probes).astype(np.float32)
    name = f"csr-{n_probes}x({pairs_per_row}p+{small_per_row})" + ("-sorted" if sort_rows else "")
    prob = Problem(name + ("-pinned" if pinned else ""), n, h, probes, bs, csr=csr)
    return _pin(prob) if pinned else prob


_INTER = np.asarray([[1, -1, 0, 0], [-1, 1, 0, 0], [0, 0, 1, -1], [0, 0, -1, 1]], np.float32)  # zero row / column sums


def quad_problem(n, seed, as_csr=False, linked=0.1):
    """Every site is probe and ballast at once, for the from-scratch energies and the Wolff rule.  Sites g, g + n/4,
    g + n/2, g + 3n/4 form a group that holds one spin, so its members lie in different lanes and super-chunks of a
    row.  Inside a group J = -A, -A, +2A along the pairings (0,1)(2,3) / (0,2)(1,3) / (0,3)(1,2): every member's big
    products cancel, and the -A bonds form a 4-cycle that a Wolff cluster always follows (1 - exp(-2A/T) is 1 in
    fp32), so groups flip whole and the cancellation survives every cluster move.  One group pair in ten carries a
    block a * [[1,-1,0,0],[-1,1,0,0],[0,0,1,-1],[0,0,-1,1]] (zero row and column sums); everything else is randn.
    Every row sum is O(sqrt n) and order sensitive, none dominates X = sum_i mv_i s_i.  n a multiple of 4."""
    assert n % 4 == 0
    rng = np.random.RandomState(seed)
    m = n // 4
    G = np.triu(rng.randn(n, n), 1).astype(np.float32)
    J = G + G.T
    member = np.arange(m)[:, None] + m * np.arange(4)[None, :]          # [group, member]
    A = np.abs(_big(rng, m))
    for (k, l), f in (((0, 1), -1.0), ((2, 3), -1.0), ((0, 2), -1.0), ((1, 3), -1.0), ((0, 3), 2.0), ((1, 2), 2.0)):
        J[member[:, k], member[:, l]] = J[member[:, l], member[:, k]] = (np.float32(f) * A).astype(np.float32)
    P, Q = np.nonzero(np.triu(rng.rand(m, m) < linked, 1))
    a = _big(rng, len(P))
    for k in range(4):
        for l in range(4):
            if _INTER[k, l] != 0:
                J[member[P, k], member[Q, l]] = J[member[Q, l], member[P, k]] = a * _INTER[k, l]
    h = rng.randn(n).astype(np.float32)
    name = f"quad-{'csr' if as_csr else 'dense'}-n{n}"
    if as_csr:
        return Problem(name, n, h, np.arange(n), np.zeros(n, np.int8), csr=to_csr(J))
    return Problem(name, n, h, np.arange(n), np.zeros(n, np.int8), J=J)


def quad_spins(n, R, seed):
    """[R, n] spins for quad_problem: the four members of a group equal, every replica its own."""
    return np.tile(np.random.RandomState(seed).choice([-1, 1], (R, n // 4)), (1, 4)).astype(np.int8)


def chain_energy(prob, s, order="canonical"):
    """E = -1/2 fp32(X) - fp32(Y) (include/sga.h, sga_recompute_energies) with mv_i the fp32 row sum in `order` and
    X = sum_i mv_i s_i, Y = sum_i h_i s_i in the energy kernels' order (exact_energy.canonical_x)."""
    import exact_energy as xe
    mv = np.concatenate([prob.row_sums(np.arange(i0, min(prob.n, i0 + 512)),
                                       np.repeat(np.asarray(s)[None, :], min(prob.n, i0 + 512) - i0, 0), order)
                         for i0 in range(0, prob.n, 512)])
    X, Y = xe.canonical_x(mv, s), xe.canonical_x(prob.h.astype(np.float64), s)
    return -0.5 * float(np.float32(X)) - float(np.float32(Y))


def gaussian_problem(n, seed):
    """What the older tests draw: randn couplings and nothing else (the record of the gap)."""
    rng = np.random.RandomState(seed)
    G = np.triu(rng.randn(n, n), 1).astype(np.float32)
    return Problem(f"randn-n{n}", n, rng.randn(n).astype(np.float32), np.arange(n), np.zeros(n, np.int8), J=G + G.T)


def to_csr(J):
    J = np.asarray(J, np.float32)
    r, c = np.nonzero(J)
    rowptr = np.concatenate([[0], np.cumsum((J != 0).sum(1))]).astype(np.int32)
    return rowptr, c.astype(np.int32), J[r, c].astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# the problems and runs that tests/test_summation_order_host.py and tests/test_summation_order_gpu.py share
# ---------------------------------------------------------------------------------------------------------------
PROBLEMS = {
    # dense: one, three, five and six super-chunks; n not a multiple of 4 or 1024, n > 2048
    "d700": lambda pinned: dense_problem(700, 11, pinned),
    "d2501": lambda pinned: dense_problem(2501, 12, pinned),
    "d5000": lambda pinned: dense_problem(5000, 13, pinned),
    "d6002": lambda pinned: dense_problem(6002, 14, pinned),
    # CSR: probe rows of at most 8, at most 64, 65 .. 512 and more than 512 entries (lanes add several entries)
    "c8": lambda pinned: csr_problem(400, 3, 2, 21, pinned),
    "c64": lambda pinned: csr_problem(400, 24, 16, 22, pinned),
    "c64-sorted": lambda pinned: csr_problem(400, 24, 16, 23, pinned, sort_rows=True),
    "c300": lambda pinned: csr_problem(360, 100, 100, 24, pinned),
    "c1200": lambda pinned: csr_problem(600, 450, 300, 25, pinned),
}
_cache = {}


def problem(key, pinned):
    if (key, pinned) not in _cache:
        if len(_cache) >= 4:
            _cache.pop(next(iter(_cache)))
        _cache[(key, pinned)] = PROBLEMS[key](pinned)
    return _cache[(key, pinned)]


METROPOLIS, GLAUBER, HEAT_BATH = 0, 1, 2
# kind: "replay" = recorded probe sites and uniforms on the problem without pinning fields; "philox" = the Philox
# stream, traced; "sequential" = sites 0 .. n-1 with recorded uniforms; "production" = the Philox stream without
# per-update records (the production kernel builds).  The last three need the pinning fields.
RUNS = {
    # name: (problem, kind, replicas, sweeps, seed, rule)
    "d700-replay": ("d700", "replay", 3, 3, 101, METROPOLIS),
    "d700-philox": ("d700", "philox", 3, 3, 102, METROPOLIS),
    "d700-glauber": ("d700", "philox", 3, 2, 103, GLAUBER),
    "d700-heat-bath": ("d700", "replay", 3, 2, 104, HEAT_BATH),
    "d700-sequential": ("d700", "sequential", 3, 2, 105, METROPOLIS),
    "d700-production": ("d700", "production", 4, 32, 106, METROPOLIS),
    "d2501-philox": ("d2501", "philox", 3, 2, 111, METROPOLIS),
    "d2501-replay": ("d2501", "replay", 2, 2, 112, METROPOLIS),
    "d2501-production": ("d2501", "production", 3, 8, 113, METROPOLIS),
    "d5000-philox": ("d5000", "philox", 2, 2, 121, METROPOLIS),
    "d5000-production": ("d5000", "production", 2, 6, 122, METROPOLIS),
    "d6002-philox": ("d6002", "philox", 2, 2, 131, METROPOLIS),
    "d6002-production": ("d6002", "production", 2, 4, 132, METROPOLIS),
    "c8-philox": ("c8", "philox", 4, 3, 201, METROPOLIS),
    "c8-production": ("c8", "production", 4, 48, 202, METROPOLIS),
    "c64-philox": ("c64", "philox", 4, 3, 211, METROPOLIS),
    "c64-replay": ("c64", "replay", 4, 3, 212, GLAUBER),
    "c64-production": ("c64", "production", 4, 32, 213, METROPOLIS),
    "c64-sorted-philox": ("c64-sorted", "philox", 4, 3, 214, METROPOLIS),
    "c64-sorted-production": ("c64-sorted", "production", 4, 32, 215, METROPOLIS),
    "c300-philox": ("c300", "philox", 4, 3, 221, METROPOLIS),
    "c300-production": ("c300", "production", 4, 32, 222, METROPOLIS),
    "c1200-philox": ("c1200", "philox", 3, 2, 231, METROPOLIS),
    "c1200-production": ("c1200", "production", 3, 16, 232, METROPOLIS),
}


def run_setup(name):
    """Everything a run of RUNS needs besides the engine: problem, initial spins, temperatures, sites, uniforms."""
    import oracle
    key, kind, R, ns, seed, rule = RUNS[name]
    prob = problem(key, kind != "replay")
    n = prob.n
    scale = prob.probe_scale()
    temps = scale * np.geomspace(2.0, 0.25, R) if R > 1 else np.asarray([scale])
    rng = np.random.RandomState(seed)
    per = ns * n
    site = u = None
    if kind == "replay":
        site = prob.probes[rng.randint(0, len(prob.probes), (R, per))].astype(np.int32)
        u = rng.rand(R, per).astype(np.float32)
    elif kind == "sequential":
        u = rng.rand(R, per).astype(np.float32)
    mode = {"replay": oracle.SITE_REPLAY, "sequential": oracle.SITE_SEQUENTIAL}.get(kind, oracle.SITE_RANDOM)
    return dict(name=name, prob=prob, kind=kind, R=R, ns=ns, seed=seed, rule=rule, temps=temps, site=site, u=u,
                mode=mode, s0=prob.s0(R, seed))


def oracle_run(cfg, energy=None):
    """The oracle's traced run of a run_setup(): its result dict, with the final spins under "spins"."""
    import oracle
    s = cfg["s0"].copy()
    ref = oracle.sweeps(cfg["prob"].oracle_problem(), s, cfg["temps"], cfg["ns"], site_mode=cfg["mode"],
                        rule=cfg["rule"], seed=cfg["seed"], replay_site=cfg["site"], replay_u=cfg["u"], trace=True,
                        energy=energy, n_threads=8)
    ref["spins"] = s
    return ref


# ---------------------------------------------------------------------------------------------------------------
# the single-site rules on a given local field (the exp recipe is the oracle's: it is not what these tests pin)
# ---------------------------------------------------------------------------------------------------------------
def _oracle():
    import oracle
    return oracle


def _expf(x):
    return np.asarray([_oracle().expf(float(v)) for v in np.asarray(x, np.float32)], np.float32)


def decide(rule, s_i, field, T, u):
    """(accepted, dE record) of proposals with local field `field` (float64) at spins s_i, as the reference's
    single-site rules decide them (core/spin_dynamics.py:131-191; oracle/sg_oracle.c cites the lines)."""
    dE = 2.0 * s_i * field
    with np.errstate(over="ignore", divide="ignore"):
        if rule == METROPOLIS:
            acc = dE <= 0.0
            up = np.nonzero(~acc)[0]
            acc[up] = u[up] < _expf((-dE[up] / T).astype(np.float32))
            return acc, np.where(acc, dE, 0.0)
        x = (-2.0 * field / T) if rule == GLAUBER else ((-2.0 * (1.0 / T)) * field)
        prob_up = np.float32(1.0) / (np.float32(1.0) + _expf(x.astype(np.float32)))
        acc = np.where(u < prob_up, 1, -1) != s_i
        return acc, np.where(acc, -dE if rule == HEAT_BATH else dE, 0.0)
