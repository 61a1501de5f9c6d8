"""Simulated quantum annealing: path-integral Monte Carlo of the transverse-field Ising model on the GPU.

H = -1/2 s J s - h s - Gamma sum_i sigma^x_i at temperature T maps (Suzuki-Trotter, P slices) onto P classical copies
of the problem, each at temperature P T, with a ferromagnetic coupling k_perp = -(P T / 2) ln tanh(Gamma / (P T))
between the same site of neighbouring copies, periodic in imaginary time (Santoro et al. 2002; Heim et al. 2015).  The
copies are the engine's replicas: AnnealEngine.sweep_transverse (sga_sweep_transverse) sweeps the even slices under
h + k_perp (s_up + s_dn), then the odd ones, with no host round trip; the tracked energies stay the slices' classical
energies, so the best over all slices is a solution of the classical problem.  overlaps() between slices works as for
any replicas.

The step serves one-model sparse (CSR) problems with integer couplings under the Metropolis rule; any other problem
raises AnnealingError with the engine's reason -- there is no classical fallback.
"""
import time
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import _native as N
from .engine import AnnealEngine
from .exceptions import ConfigurationError
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

    def __post_init__(self):
        self.check()

    def check(self):
        for name in ("n_slices", "n_instances", "n_sweeps", "measure_interval"):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or v < 1:
                raise ConfigurationError(f"{name} must be a positive integer")
        if self.n_slices < 2 or self.n_slices % 2 != 0:
            raise ConfigurationError("n_slices must be an even number of at least 2 (the slices move in two halves)")
        if not np.isfinite(self.temperature) or self.temperature <= 0:
            raise ConfigurationError("temperature must be positive and finite")
        if not isinstance(self.transverse_field, TransverseField):
            raise ConfigurationError("transverse_field must be a TransverseField")

    def couplings(self) -> np.ndarray:
        """float32 [n_sweeps]: k_perp per sweep."""
        k = transverse_coupling(self.transverse_field.gammas(self.n_sweeps), self.temperature, self.n_slices)
        k32 = np.asarray(k, np.float64).astype(np.float32)
        if not np.all(np.isfinite(k32)):
            raise ConfigurationError("the schedule gives an infinite k_perp (a transverse field too close to 0)")
        return k32


class SimulatedQuantumAnnealing:
    def __init__(self, config: SimulatedQuantumAnnealingConfig):
        config.check()
        self.config = config
        self.final_energies = None   # float64 [n_instances, n_slices]: the slices' classical energies at the end
        self.slice_overlaps = None   # int32 [R, R] of run(measure_overlaps=True): s_a . s_b between the final slices
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.use_cuda = self.device.type == "cuda"

    def run(self, model: IsingModel, measure_overlaps: bool = False) -> AnnealingResult:
        cfg = self.config
        cfg.check()
        P, G, n = int(cfg.n_slices), int(cfg.n_instances), model.n_spins
        R = P * G
        k = cfg.couplings()
        gam = cfg.transverse_field.gammas(cfg.n_sweeps)
        dev_idx = cfg.device_index if cfg.device_index is not None else _device_index(model.device)
        t_start = time.time()
        energy_history, temp_history, acc_history = [], [], []
        step = int(cfg.measure_interval)
        with AnnealEngine(dev_idx) as eng:
            model.load_into(eng)
            eng.init_replicas(R, seed=fresh_seed(cfg.seed))
            eng.set_temperatures(P * float(cfg.temperature))
            acc_prev = np.zeros(R, np.int64)
            for k0 in range(0, int(cfg.n_sweeps), step):
                ns = min(step, int(cfg.n_sweeps) - k0)
                eng.sweep_transverse(ns, P, k[k0:k0 + ns])
                en, acc, _ = eng.snapshot(slots=False)
                energy_history.append(float(en.min()))       # the lowest classical energy over the slices now
                temp_history.append(float(gam[k0 + ns - 1]))  # (the transverse field: T is constant)
                acc_history.append(float((acc - acc_prev).sum()) / float(R * n * ns))
                acc_prev = acc
            self.final_energies = eng.energies().reshape(G, P)
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
                 final_field_strength: float = 0.01, n_instances: int = 1):
        self.base_annealer = base_annealer
        self.n_instances = int(n_instances)
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
            device_index=self._base("device_index", None))
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
