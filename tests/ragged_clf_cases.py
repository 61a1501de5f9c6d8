"""Shared problems of the ragged cached-field tests (option "ragged_field_cache"): two batches of sparse models of
different sizes, their per-model temperature ladders and the CPU oracle run on EACH MODEL ALONE with replica0 = m * k --
the reference every test compares against.  The shapes are the smallest at which the ragged kernel can go wrong:

  batch S (short rows: four waves per replica, one entry per thread)
    0  n = 3     complete                      smaller than one window, smaller than a wave
    1  n = 37    p = 0.3, half-integer h       odd n; makes the batch-wide scale 2 for the integer-h models beside it
    2  n = 100   p = 0.9 (rows ~ 90 entries)   rows longer than one wave
    3  n = 257   p = 0.05                      n = 1 mod 32
    4  n = 700   mean degree 12                512 + 188 updates: two super-windows at four waves, the second partial
    5  n = 1201  p = 0.007, |J| <= 3           the largest model (n_max), integer h, |J| > 1
  batch L (a row of more than 512 entries: eight waves per replica, two entries per thread)
    S's models 0, 1 and 3, then n = 1500 with p = 0.4 (rows of ~ 600 entries)

k = 3 replicas per model, one ladder per model from hot to cold, scaled by the model's typical field so that the hot
replica accepts most proposals and the cold one few (checked on the CPU from the oracle's counters: check_acceptance).
Nothing here needs a GPU.  The cached problems and references are shared: callers must not write into them."""
import functools

import numpy as np

import oracle

K = 3          # replicas per model
SEED = 20260
N_SWEEPS = 4   # production sweeps of the parity test


def sym_sparse(n, density, seed, jmax=1):
    """Symmetric sparse integer J with a zero diagonal as CSR with strictly sorted rows; |J| in 1..jmax."""
    rng = np.random.RandomState(seed)
    mask = np.triu(rng.rand(n, n) < density, 1)
    v = (rng.randint(1, jmax + 1, (n, n)) * (rng.randint(0, 2, (n, n)) * 2 - 1)).astype(np.float32)
    J = np.where(mask, v, 0).astype(np.float32)
    J = J + J.T
    return dense_to_csr(J)


def dense_to_csr(J):
    n = J.shape[0]
    nz = J != 0
    rowptr = np.concatenate([[0], np.cumsum(nz.sum(1))]).astype(np.int32)
    colidx = np.nonzero(nz)[1].astype(np.int32)
    val = J[nz].astype(np.float32)
    assert rowptr[-1] == colidx.size == val.size and rowptr.size == n + 1
    return rowptr, colidx, val


def fields(n, seed, half=False):
    h = np.random.RandomState(seed).randint(-2, 3, n).astype(np.float32)
    return h / 2 if half else h


# (n, density, max |J|, half-integer h)
_S = [(3, 1.0, 1, False), (37, 0.3, 1, True), (100, 0.9, 1, False), (257, 0.05, 1, False), (700, 12.0 / 699.0, 1, False),
      (1201, 0.007, 3, False)]


@functools.lru_cache(maxsize=None)
def _model(idx):
    if idx == "long":
        return sym_sparse(1500, 0.4, 777) + (fields(1500, 778),)
    n, d, jmax, half = _S[idx]
    if idx == 0:  # odd h beside +-1 couplings: no site of the triangle ever has a zero field (no free flips when cold)
        return sym_sparse(n, d, 100, jmax) + (np.asarray([1.0, -1.0, 1.0], np.float32),)
    return sym_sparse(n, d, 100 + idx, jmax) + (fields(n, 200 + idx, half),)


@functools.lru_cache(maxsize=None)
def batch(name):
    """The models of batch "S" | "L" as a tuple of (rowptr, colidx, val, h)."""
    if name == "S":
        return tuple(_model(i) for i in range(len(_S)))
    assert name == "L"
    return (_model(0), _model(1), _model(3), _model("long"))


def sizes(probs):
    return [len(p[0]) - 1 for p in probs]


def longest_row(probs):
    return max(int(np.diff(p[0]).max()) for p in probs)


def model_ladder(p, k=K, hot=6.0, cold=0.25):
    """k temperatures from hot to cold in units of the model's typical field sqrt(sum_j J_ij^2 + h_i^2)."""
    n = len(p[0]) - 1
    unit = max(1.0, float(np.sqrt((np.sum(p[2].astype(np.float64) ** 2) + np.sum(p[3].astype(np.float64) ** 2)) / n)))
    return np.asarray([unit * hot * (cold / hot) ** (i / max(k - 1, 1)) for i in range(k)])


def ladders(probs, k=K, **kw):
    return np.concatenate([model_ladder(p, k, **kw) for p in probs])


class OracleBatch:
    """The CPU oracle on each model alone: model m's k replicas carry the global indices m k ... m k + k - 1 as their
    Philox key.  Follows a run stage by stage (sweeps, set_spins, new temperatures); energies, bests and counters carry
    over as they do in an engine."""

    def __init__(self, probs, temps, k=K, seed=SEED, spins=None):
        self.k, self.seed, self.sweep0 = k, seed, 0
        self.probs = [oracle.Problem(csr=p[:3], h=p[3]) for p in probs]
        self.sizes = sizes(probs)
        self.temps = np.asarray(temps, np.float64).copy()
        self.spins = [oracle.init_spins(n, k, seed, replica0=m * k) if spins is None else spins[m].copy()
                      for m, n in enumerate(self.sizes)]
        self.energy = [np.asarray(oracle.energy(pr, s), np.float64) for pr, s in zip(self.probs, self.spins)]
        self.best_energy = [e.copy() for e in self.energy]
        self.best_spins = [s.copy() for s in self.spins]
        self.n_accepted = [np.zeros(k, np.int64) for _ in self.probs]

    def sweep(self, ns, **kw):
        """ns sweeps of every model; returns the energy trace [ns, M k]."""
        traces = []
        for m, pr in enumerate(self.probs):
            sl = slice(m * self.k, (m + 1) * self.k)
            old_best = self.best_energy[m]
            ref = oracle.sweeps(pr, self.spins[m], self.temps[sl], ns, seed=self.seed, sweep0=self.sweep0,
                                replica0=m * self.k, energy=self.energy[m], best_energy=old_best, **kw)
            self.energy[m] = ref["energy"]
            better = ref["best_energy"] < old_best  # (the oracle starts its best spins from the current ones)
            self.best_spins[m] = np.where(better[:, None], ref["best_spins"], self.best_spins[m])
            self.best_energy[m] = ref["best_energy"]
            self.n_accepted[m] = self.n_accepted[m] + ref["n_accepted"]
            traces.append(ref["energy_trace"])
        self.sweep0 += ns
        return np.concatenate(traces, axis=1)

    def set_spins(self, r, s):
        """An engine's sga_set_spins: new spins, energy from scratch, the replica's best reset to them."""
        m, j = divmod(r, self.k)
        self.spins[m][j] = s
        e = float(oracle.energy(self.probs[m], self.spins[m][j]))
        self.energy[m] = self.energy[m].copy()
        self.energy[m][j] = e
        self.best_energy[m] = self.best_energy[m].copy()
        self.best_energy[m][j] = e
        self.best_spins[m] = self.best_spins[m].copy()
        self.best_spins[m][j] = s

    def exchange(self, round_=0):
        """One neighbour exchange round per model ladder (temperatures move, spins stay); returns the swaps."""
        R = self.k * len(self.probs)
        if not hasattr(self, "slot_temps"):
            self.slot_temps = self.temps.copy()
            self.slot_to_rep = np.arange(R, dtype=np.int32)
        swaps = 0
        full_e = np.concatenate(self.energy)
        for m in range(len(self.probs)):
            sl = slice(m * self.k, (m + 1) * self.k)
            view = self.slot_to_rep[sl].copy()
            e_m = np.zeros(R)
            e_m[sl] = full_e[sl]
            swaps += oracle.pt_exchange_round(self.slot_temps[sl], e_m, view, seed=self.seed, round_=round_, ladder=m)
            self.slot_to_rep[sl] = view
        for slot, rep in enumerate(self.slot_to_rep):
            self.temps[rep] = self.slot_temps[slot]
        return swaps

    def padded_spins(self, which="spins"):
        rows = self.spins if which == "spins" else self.best_spins
        out = np.zeros((self.k * len(self.probs), max(self.sizes)), np.int8)
        for m, s in enumerate(rows):
            out[m * self.k:(m + 1) * self.k, :self.sizes[m]] = s
        return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """Batch `name` after N_SWEEPS production sweeps on its ladders: (OracleBatch, energy trace).  Shared: read only."""
    probs = batch(name)
    ob = OracleBatch(probs, ladders(probs))
    trace = ob.sweep(N_SWEEPS)
    return ob, trace


def check_acceptance(name):
    """The condition on the inputs: over the reference run every model with n >= 37 accepts some proposals and rejects
    some -- in its hot replica most, in its cold one fewer -- so that both the accept path and the reject path of the
    cached-field kernel are walked in every model.  Returns the per-replica acceptance."""
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
