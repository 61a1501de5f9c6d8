"""Simulated quantum annealing: path-integral Monte Carlo of the transverse-field Ising model on the GPU.

H = -1/2 s J s - h s - Gamma sum_i sigma^x_i at temperature T maps (Suzuki-Trotter, P slices) onto P classical copies
of the problem, each at temperature P T, with a ferromagnetic coupling k_perp = -(P T / 2) ln tanh(Gamma / (P T))
between the same site of neighbouring copies, periodic in imaginary time (Santoro et al. 2002; Heim et al. 2015).  The
copies are the engine's replicas: AnnealEngine.sweep_transverse (sga_sweep_transverse) sweeps the even slices under
h + k_perp (s_up + s_dn), then the odd ones, with no host round trip; the tracked energies stay the slices' classical
energies, so the best over all slices is a solution of the classical problem.  overlaps() between slices works as for
any replicas.

At small Gamma k_perp grows without bound and a single-slice flip against two equal neighbours is never accepted: the
slices freeze into identical copies.  AnnealEngine.worldline_clusters (sga_worldline_clusters) is the move that keeps
the method ergodic there: at each site the ring of slices is cut into segments by bonds drawn with probability
bond_probability(k_perp, P T) between equal neighbouring slices, and each segment flips as one under the classical
field (Rieger and Kawashima 1999; Heim et al. 2015).  SimulatedQuantumAnnealingConfig(worldline_clusters=True) follows
every cluster_interval-th transverse sweep with one such sweep.

The step serves one-model sparse (CSR) problems with integer couplings under the Metropolis rule; any other problem
raises AnnealingError with the engine's reason -- there is no classical fallback.

Dense couplings (SK glasses, number partitioning, dense QUBO encodings) are an opt-in:
SimulatedQuantumAnnealingConfig(dense_couplings=True) hands the model to the engine as one dense matrix with the field
cache on and sweeps through AnnealEngine.sweep_transverse_dense (sga_sweep_transverse_dense) -- the same step, a slice's
local fields resident in LDS and a coupling row read on accept only.  It serves integer symmetric J with a zero diagonal
and h in multiples of 1/2; with fixed_point_fields=True beside it (engine option "clf_fixed_point") also real-valued J on
a binary grid -- a QUBO's Q / 4, quarter-valued penalty encodings -- and any h, the fields kept as exact fixed point
(int32 | int64).  The cluster move beside it is a flag of its own, dense_worldline_clusters=True: every
cluster_interval-th dense sweep is followed by AnnealEngine.worldline_clusters_dense (sga_worldline_clusters_dense), the
same cluster step decided on the same cached fields, which stay valid between the two calls.

The quantum side of a run is a function of one integer per instance, the number B of broken time links
(AnnealEngine.time_links, sga_get_time_links): transverse_magnetization gives <sigma^x> and quantum_energy the energy
estimator of H.  The same count decides the replica exchange along Gamma (quantum parallel tempering):
SimulatedQuantumAnnealingConfig(field_ladder=[c_0, ...], field_exchange_interval=m) runs instance g at c_g Gamma(t) and
follows every m-th sweep with one round of AnnealEngine.exchange_transverse (sga_exchange_transverse) between neighbouring
instances, whole instances trading places on the device.
"""
import time
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native as N
from .engine import AnnealEngine
from .exceptions import AnnealingError, ConfigurationError
from .gpu_annealer import fresh_seed
from .ising_model import IsingModel, _device_index
from .result import AnnealingResult


def transverse_coupling(gamma, temperature: float, n_slices: int):
    """k_perp = -(P T / 2) ln tanh(Gamma / (P T)) in classical energy units: positive, decreasing in Gamma, +inf at
    Gamma = 0 and -> 0 as Gamma -> inf.  gamma: a scalar or an array (float64 out)."""
    P = int(n_slices)
    if P < 2 or P % 2 != 0:
        raise ConfigurationError("n_slices must be an even number of at least 2")
    if not np.isfinite(temperature) or temperature <= 0:
        raise ConfigurationError("temperature must be positive and finite")
    g = np.asarray(gamma, np.float64)
    if np.any(np.isnan(g)) or np.any(g < 0):
        raise ConfigurationError("gamma must not be negative")
    pt = P * float(temperature)
    with np.errstate(divide="ignore"):
        k = -0.5 * pt * np.log(np.tanh(g / pt))
    k = np.where(k == 0.0, 0.0, k)  # (tanh rounds to 1 for a large Gamma: +0, not -0)
    return float(k) if k.ndim == 0 else k


def bond_probability(k_perp, slice_temperature: float):
    """p_bond = 1 - exp(-2 k_perp / T) = -expm1(-2 k / T) in float64: the probability of a bond between two equal spins
    of neighbouring slices that run at temperature T (= P times the quantum temperature) under the coupling k_perp.  With
    it one site update of AnnealEngine.worldline_clusters satisfies detailed balance against exp(-H_eff / T).  k_perp:
    a scalar or an array; a negative one has no such clusters (an antiferromagnetic time coupling)."""
    if not np.isfinite(slice_temperature) or slice_temperature <= 0:
        raise ConfigurationError("slice_temperature must be positive and finite")
    k = np.asarray(k_perp, np.float64)
    if np.any(np.isnan(k)) or np.any(k < 0):
        raise ConfigurationError("k_perp must not be negative: an antiferromagnetic time coupling has no such clusters")
    b = -np.expm1(-2.0 * k / float(slice_temperature))
    return float(b) if b.ndim == 0 else b


def transverse_magnetization(links, n_spins, n_slices, gamma, temperature):
    """<sigma^x> per site of a path-integral configuration with B = links broken time links out of n P:
    [(n P - B) tanh(a) + B / tanh(a)] / (n P), a = Gamma / (P T), in float64 -- tanh(a) for identical slices, 1 / tanh(a)
    with every link broken.  Arrays broadcast against each other."""
    B = np.asarray(links, np.float64)
    nP = np.asarray(n_spins, np.float64) * np.asarray(n_slices, np.float64)
    t = np.tanh(np.asarray(gamma, np.float64) / (np.asarray(n_slices, np.float64) * np.asarray(temperature, np.float64)))
    m = ((nP - B) * t + B / t) / nP
    return float(m) if m.ndim == 0 else m


def quantum_energy(slice_energies, links, n_spins, n_slices, gamma, temperature):
    """The estimator of <H> = <H_classical> - Gamma sum_i <sigma^x_i>: the mean over the slices of the classical energies
    slice_energies [G, P] (or [P]) minus Gamma n transverse_magnetization(links, ...), float64 [G] (or a scalar)."""
    E = np.asarray(slice_energies, np.float64).mean(axis=-1)
    q = E - np.asarray(gamma, np.float64) * np.asarray(n_spins, np.float64) * \
        transverse_magnetization(links, n_spins, n_slices, gamma, temperature)
    return float(q) if np.ndim(q) == 0 else q


@dataclass
class TransverseField:
    """Gamma per sweep.  schedule: 'linear_decrease' (initial -> final in equal steps), 'geometric_decrease' (equal
    ratios; final > 0) or 'constant' (initial throughout)."""
    schedule: str = "linear_decrease"
    initial: float = 5.0
    final: float = 0.01

    def __post_init__(self):
        if self.schedule not in ("linear_decrease", "geometric_decrease", "constant"):
            raise ConfigurationError("schedule must be 'linear_decrease', 'geometric_decrease' or 'constant'")
        if not np.isfinite(self.initial) or self.initial <= 0:
            raise ConfigurationError("the initial transverse field must be positive and finite")
        if self.schedule != "constant":
            if not np.isfinite(self.final) or self.final <= 0 or self.final > self.initial:
                raise ConfigurationError("the final transverse field must be positive and at most the initial one "
                                         "(Gamma = 0 freezes the slices together: k_perp diverges)")

    def gammas(self, n_sweeps: int) -> np.ndarray:
        """float64 [n_sweeps]."""
        n = int(n_sweeps)
        if n < 1:
            raise ConfigurationError("n_sweeps must be a positive integer")
        if self.schedule == "constant":
            return np.full(n, float(self.initial))
        x = np.arange(n, dtype=np.float64) / max(n - 1, 1)
        if self.schedule == "linear_decrease":
            return self.initial + (self.final - self.initial) * x
        return self.initial * (self.final / self.initial) ** x


@dataclass
class SimulatedQuantumAnnealingConfig:
    n_slices: int = 32                    # P: Trotter slices per instance (even)
    n_instances: int = 1                  # G: independent instances side by side (R = G P replicas)
    temperature: float = 0.1              # T of the quantum system; every slice runs at P T
    n_sweeps: int = 1000
    transverse_field: TransverseField = field(default_factory=TransverseField)
    seed: Optional[int] = None
    measure_interval: int = 1             # sweeps per engine call; the histories hold one record per call
    device_index: Optional[int] = None
    worldline_clusters: bool = False      # follow transverse sweeps with world-line cluster sweeps (sga_worldline_clusters)
    cluster_interval: int = 1             # ... every cluster_interval-th of them
    dense_couplings: bool = False         # hand the model over as one dense matrix, field cache on, and sweep through
    #                                       sga_sweep_transverse_dense (False: the model's own form, CSR rows served only)
    dense_worldline_clusters: bool = False  # with dense_couplings: follow every cluster_interval-th dense sweep with one
    #                                         cluster sweep on the cached fields (sga_worldline_clusters_dense)
    field_ladder: Optional[Sequence[float]] = None  # multipliers c_g, one per instance: instance g runs at c_g Gamma(t)
    field_exchange_interval: int = 0      # m > 0: every m-th sweep, counted over the run, is followed by one round of
    #                                       replica exchange between neighbouring instances (sga_exchange_transverse)
    fixed_point_fields: bool = False      # with dense_couplings: engine option "clf_fixed_point" -- dense models the integer
    #                                       cached-field form does not take (real-valued J on a binary grid, any h) are
    #                                       swept on exact fixed-point fields; the cluster move does not serve those

    def __post_init__(self):
        self.check()

    def check(self):
        for name in ("n_slices", "n_instances", "n_sweeps", "measure_interval", "cluster_interval"):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or v < 1:
                raise ConfigurationError(f"{name} must be a positive integer")
        if self.n_slices < 2 or self.n_slices % 2 != 0:
            raise ConfigurationError("n_slices must be an even number of at least 2 (the slices move in two halves)")
        if not np.isfinite(self.temperature) or self.temperature <= 0:
            raise ConfigurationError("temperature must be positive and finite")
        if not isinstance(self.transverse_field, TransverseField):
            raise ConfigurationError("transverse_field must be a TransverseField")
        if not isinstance(self.worldline_clusters, (bool, np.bool_)):
            raise ConfigurationError("worldline_clusters must be True or False")
        if self.worldline_clusters and self.n_slices > 64:
            raise ConfigurationError("world-line clusters serve at most 64 slices (one lane of a wave per slice)")
        if not isinstance(self.dense_couplings, (bool, np.bool_)):
            raise ConfigurationError("dense_couplings must be True or False")
        if not isinstance(self.dense_worldline_clusters, (bool, np.bool_)):
            raise ConfigurationError("dense_worldline_clusters must be True or False")
        if self.dense_worldline_clusters:
            self.check_dense_clusters()
        if not isinstance(self.fixed_point_fields, (bool, np.bool_)):
            raise ConfigurationError("fixed_point_fields must be True or False")
        if self.fixed_point_fields and not self.dense_couplings:
            raise ConfigurationError("fixed_point_fields needs dense_couplings=True (the transverse sweep on sparse rows keeps "
                                     "no cached fields)")
        if self.field_ladder is not None:
            c = np.asarray(self.field_ladder, np.float64)
            if c.ndim != 1 or c.size != int(self.n_instances):
                raise ConfigurationError("field_ladder must hold one multiplier per instance (n_instances values)")
            if not np.all(np.isfinite(c)) or np.any(c <= 0):
                raise ConfigurationError("field_ladder must hold positive finite multipliers")
        m = self.field_exchange_interval
        if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or m < 0:
            raise ConfigurationError("field_exchange_interval must be a non-negative integer (0: no exchange)")
        if m > 0 and self.n_instances < 2:
            raise ConfigurationError("field_exchange_interval needs n_instances >= 2 (an exchange is between two instances)")

    def check_dense_clusters(self):
        """What dense_worldline_clusters asks of the rest of the configuration."""
        if not self.dense_couplings:
            raise ConfigurationError("dense_worldline_clusters needs dense_couplings=True (sparse models: worldline_clusters)")
        if self.n_slices > 64:
            raise ConfigurationError("world-line clusters serve at most 64 slices (one lane of a wave per slice)")

    def couplings(self) -> np.ndarray:
        """float32 [n_sweeps]: k_perp per sweep."""
        k = transverse_coupling(self.transverse_field.gammas(self.n_sweeps), self.temperature, self.n_slices)
        k32 = np.asarray(k, np.float64).astype(np.float32)
        if not np.all(np.isfinite(k32)):
            raise ConfigurationError("the schedule gives an infinite k_perp (a transverse field too close to 0)")
        return k32

    def couplings_by_instance(self) -> np.ndarray:
        """float32 [n_sweeps, n_instances]: k_perp per sweep and instance, instance g at field_ladder[g] Gamma(t) (no
        ladder: every column is couplings())."""
        c = np.ones(int(self.n_instances)) if self.field_ladder is None else np.asarray(self.field_ladder, np.float64)
        g = self.transverse_field.gammas(self.n_sweeps)[:, None] * c[None, :]
        k32 = np.asarray(transverse_coupling(g, self.temperature, self.n_slices), np.float64).astype(np.float32)
        if not np.all(np.isfinite(k32)):
            raise ConfigurationError("the schedule gives an infinite k_perp (a transverse field too close to 0)")
        return k32


class SimulatedQuantumAnnealing:
    def __init__(self, config: SimulatedQuantumAnnealingConfig):
        config.check()
        self.config = config
        self.final_energies = None   # float64 [n_instances, n_slices]: the slices' classical energies at the end
        self.slice_overlaps = None   # int32 [R, R] of run(measure_overlaps=True): s_a . s_b between the final slices
        self.cluster_statistics = None  # int64 [3] of a run with world-line clusters: segments formed, segments flipped,
        #                                 slice spins flipped, summed over the run
        self.time_links = None       # int64 [n_instances]: the broken time links of every instance at the end
        self.transverse_magnetization = None  # float64 [n_instances]: <sigma^x> per site at the end, from time_links
        self.field_exchange_statistics = None  # of a run with field_exchange_interval > 0: (attempts, accepts), int64
        #                                        [n_instances - 1] each, per pair of neighbouring instances
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.use_cuda = self.device.type == "cuda"

    def _sweeps(self, eng, k0: int, ns: int, k, clusters: bool, dense: bool = False):
        """Transverse sweeps k0 ... k0 + ns - 1; with clusters, every cluster_interval-th one (counted over the run) is
        followed by one cluster sweep at its k_perp, drawn at round = the sweep's index.  dense: the engine holds dense
        rows, the sweeps are sweep_transverse_dense's and the cluster sweeps worldline_clusters_dense's.  k: [n_sweeps],
        or [n_sweeps, G] with a field ladder.  With field_exchange_interval = m > 0 every m-th sweep (counted over the
        run) is followed -- after its cluster sweep, if one is due -- by one exchange round at its row of k, round = the
        sweep's index, the parity alternating from 0 with the exchanges of the run."""
        cfg = self.config
        P = int(cfg.n_slices)
        sweep = eng.sweep_transverse_dense if dense else eng.sweep_transverse
        m = int(cfg.field_exchange_interval)
        if not clusters and m == 0:
            sweep(ns, P, k[k0:k0 + ns])
            return
        move = eng.worldline_clusters_dense if dense else eng.worldline_clusters
        every, slice_T = int(cfg.cluster_interval), P * float(cfg.temperature)
        t = k0
        while t < k0 + ns:
            stop = k0 + ns  # the sweeps up to and with the next one that is followed
            if clusters:
                stop = min(stop, ((t // every) + 1) * every)
            if m:
                stop = min(stop, ((t // m) + 1) * m)
            sweep(stop - t, P, k[t:stop])
            if clusters and stop % every == 0:
                row = k[stop - 1]
                b = bond_probability(float(row), slice_T) if np.ndim(row) == 0 else bond_probability(row, slice_T)[None, :]
                self.cluster_statistics += move(1, P, b, round=stop - 1, stats=True).sum(axis=0)
            if m and stop % m == 0:
                parity = (stop // m - 1) & 1
                accepted, _ = eng.exchange_transverse(P, k[stop - 1], parity=parity, round=stop - 1)
                attempts, accepts = self.field_exchange_statistics
                lower = np.arange(parity, len(attempts), 2)  # the lower instance of every pair of this round
                attempts[lower] += 1
                accepts[lower] += accepted[lower]
            t = stop

    def run(self, model: IsingModel, measure_overlaps: bool = False, worldline_clusters: Optional[bool] = None,
            dense_worldline_clusters: Optional[bool] = None) -> AnnealingResult:
        """worldline_clusters: None = the configuration's; False is the transverse sweeps alone.  dense_worldline_clusters
        likewise: the cluster move of a run with dense_couplings=True."""
        cfg = self.config
        cfg.check()
        clusters = bool(cfg.worldline_clusters if worldline_clusters is None else worldline_clusters)
        dense_clusters = bool(cfg.dense_worldline_clusters if dense_worldline_clusters is None else dense_worldline_clusters)
        if clusters and cfg.n_slices > 64:
            raise ConfigurationError("world-line clusters serve at most 64 slices (one lane of a wave per slice)")
        if cfg.dense_couplings and clusters:
            raise AnnealingError("world-line clusters are not served on dense couplings: sga_worldline_clusters reads CSR rows "
                                 "(run with dense_worldline_clusters=True, which decides the move on the cached fields, with "
                                 "dense_couplings=False on a sparse model, or without worldline_clusters)")
        if dense_clusters:
            cfg.check_dense_clusters()
            clusters = True  # (from here on: a cluster sweep follows, by whichever call the engine's rows are served)
        self.cluster_statistics = np.zeros(3, np.int64) if clusters else None
        P, G, n = int(cfg.n_slices), int(cfg.n_instances), model.n_spins
        R = P * G
        k = cfg.couplings() if cfg.field_ladder is None else cfg.couplings_by_instance()
        gam = cfg.transverse_field.gammas(cfg.n_sweeps)
        self.field_exchange_statistics = (np.zeros(G - 1, np.int64), np.zeros(G - 1, np.int64)) if cfg.field_exchange_interval else None
        dev_idx = cfg.device_index if cfg.device_index is not None else _device_index(model.device)
        t_start = time.time()
        energy_history, temp_history, acc_history = [], [], []
        step = int(cfg.measure_interval)
        with AnnealEngine(dev_idx) as eng:
            dense = False
            if cfg.dense_couplings:
                # one dense matrix with the field cache on: the rows stay dense (the sparse route is taken with the cache
                # off or left to the engine only); should the engine hold CSR rows all the same, they are sweep_transverse's
                eng.set_field_cache("on")
                if cfg.fixed_point_fields:
                    eng.set_option("clf_fixed_point", 1)  # (read when the couplings are set)
                J = model.couplings.to_dense() if model.couplings.is_sparse else model.couplings
                eng.set_dense(J, model.external_fields)
                rq = eng.route_query()
                dense = rq.kind != N.ROUTE_CSR
                if cfg.fixed_point_fields and dense_clusters and dense and not rq.clf_ok and rq.clf_bits in (32, 64):
                    raise AnnealingError("dense world-line clusters are not served on fixed-point fields: the model landed on "
                                         "the fixed-point cached fields (int%d), and sga_worldline_clusters_dense decides its "
                                         "segments on the integer form's fields only (run without dense_worldline_clusters, or "
                                         "with integer J and h in multiples of 1/2)" % rq.clf_bits)
            else:
                model.load_into(eng)
            eng.init_replicas(R, seed=fresh_seed(cfg.seed))
            eng.set_temperatures(P * float(cfg.temperature))
            acc_prev = np.zeros(R, np.int64)
            for k0 in range(0, int(cfg.n_sweeps), step):
                ns = min(step, int(cfg.n_sweeps) - k0)
                self._sweeps(eng, k0, ns, k, clusters, dense)
                en, acc, _ = eng.snapshot(slots=False)
                energy_history.append(float(en.min()))       # the lowest classical energy over the slices now
                temp_history.append(float(gam[k0 + ns - 1]))  # (the transverse field: T is constant)
                acc_history.append(float((acc - acc_prev).sum()) / float(R * n * ns))
                acc_prev = acc
            self.final_energies = eng.energies().reshape(G, P)
            self.time_links = eng.time_links(P)
            ladder = 1.0 if cfg.field_ladder is None else np.asarray(cfg.field_ladder, np.float64)
            self.transverse_magnetization = np.asarray(transverse_magnetization(
                self.time_links, n, P, ladder * float(gam[-1]), float(cfg.temperature)), np.float64)
            if measure_overlaps:
                self.slice_overlaps = eng.overlaps()
            best_energy, best_configuration, _ = eng.best()
        return AnnealingResult(
            best_configuration=torch.from_numpy(best_configuration.astype(np.float32)), best_energy=float(best_energy),
            energy_history=energy_history, temperature_history=temp_history, acceptance_rate_history=acc_history,
            total_time=time.time() - t_start, n_sweeps=int(cfg.n_sweeps), algorithm="simulated_quantum_annealing",
            device=f"cuda:{dev_idx}", random_seed=cfg.seed)

    def __repr__(self) -> str:
        c = self.config
        return (f"SimulatedQuantumAnnealing(n_slices={c.n_slices}, n_instances={c.n_instances}, "
                f"temperature={c.temperature}, n_sweeps={c.n_sweeps})")


class QuantumFluctuations:
    """The upstream README's entry point: quantum fluctuations added to a base annealer.  The base annealer gives the
    number of sweeps, the temperature (its final one) and the seed; the schedule gives Gamma."""

    def __init__(self, base_annealer=None, transverse_field_schedule: str = "linear_decrease", initial_field_strength: float = 5.0,
                 final_field_strength: float = 0.01, n_instances: int = 1, worldline_clusters: bool = False,
                 dense_couplings: bool = False, dense_worldline_clusters: bool = False,
                 field_ladder: Optional[Sequence[float]] = None, field_exchange_interval: int = 0,
                 fixed_point_fields: bool = False):
        self.base_annealer = base_annealer
        self.n_instances = int(n_instances)
        self.worldline_clusters = bool(worldline_clusters)
        self.dense_couplings = bool(dense_couplings)
        self.dense_worldline_clusters = bool(dense_worldline_clusters)
        self.fixed_point_fields = bool(fixed_point_fields)
        self.field_ladder = None if field_ladder is None else tuple(float(c) for c in field_ladder)
        self.field_exchange_interval = field_exchange_interval
        self.field = TransverseField(transverse_field_schedule, float(initial_field_strength),
                                     min(float(final_field_strength), float(initial_field_strength)))
        self.last = None  # the SimulatedQuantumAnnealing of the last call (final_energies, slice_overlaps)

    def _base(self, name, default):
        cfg = getattr(self.base_annealer, "config", None)
        v = getattr(cfg, name, None)
        return default if v is None else v

    def _run(self, model, P, T, tf) -> AnnealingResult:
        cfg = SimulatedQuantumAnnealingConfig(
            n_slices=int(P), n_instances=self.n_instances, temperature=float(T), n_sweeps=int(self._base("n_sweeps", 1000)),
            transverse_field=tf, seed=self._base("random_seed", None), measure_interval=int(self._base("record_interval", 10)),
            device_index=self._base("device_index", None), worldline_clusters=self.worldline_clusters,
            dense_couplings=self.dense_couplings, dense_worldline_clusters=self.dense_worldline_clusters,
            fixed_point_fields=self.fixed_point_fields, field_ladder=self.field_ladder, field_exchange_interval=self.field_exchange_interval)
        self.last = SimulatedQuantumAnnealing(cfg)
        return self.last.run(model)

    def simulated_quantum_anneal(self, model: IsingModel, n_trotter_slices: int = 32, quantum_monte_carlo: bool = True) -> AnnealingResult:
        if not quantum_monte_carlo:
            raise ConfigurationError("simulated_quantum_anneal is path-integral quantum Monte Carlo: quantum_monte_carlo=False "
                                     "has no implementation (there is no classical fallback)")
        return self._run(model, n_trotter_slices, self._base("final_temp", 0.1), self.field)

    def path_integral_mc(self, model: IsingModel, imaginary_time_slices: int = 64, quantum_temperature: float = 0.1) -> AnnealingResult:
        """Equilibrium path-integral Monte Carlo at a CONSTANT transverse field (the initial strength)."""
        return self._run(model, imaginary_time_slices, quantum_temperature, TransverseField("constant", self.field.initial))
