"""PopulationAnnealing: a population of replicas cooled together, resampled by weight at every temperature step.

Population annealing (Hukushima and Iba 2003; Machta 2010; Wang, Machta and Katzgraber 2015) is simulated annealing made
an equilibrium method: R replicas start at beta = 0 (random spins), and at every step beta -> beta' each replica is copied
or culled in proportion to exp(-(beta' - beta) E) before the population is swept at beta'.  The normalisations Q of the
steps multiply up to the partition function, so the run yields the free energy, and the number of initial replicas that
still have descendants (the families) says whether it equilibrated.

Every replica is resident on the GPU.  A step is AnnealEngine.resample (sga_resample: planned and copied on the device,
exact in integers), set_temperatures and sweep; the host keeps the family bookkeeping (family = family[parents]) and
the logarithms.  With n_populations > 1 the engine holds that many independent populations side by side -- independent
runs of one schedule, whose spread gives error bars.
"""
import time
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native as N
from .engine import AnnealEngine
from .exceptions import ConfigurationError
from .gpu_annealer import fresh_seed
from .ising_model import IsingModel, _device_index
from .result import AnnealingResult
from .spin_dynamics import UpdateRule, rule_code

MAX_POPULATION = 1 << 23  # sga_resample: the weight sum of a population stays inside 64 bits


@dataclass
class PopulationAnnealingConfig:
    population_size: int = 1024
    n_populations: int = 1                # independent populations side by side (error bars)
    betas: Optional[Sequence[float]] = None  # the inverse temperatures of the run, betas[0] == 0; None: linear, below
    beta_max: float = 1.0                 # betas None: n_steps equal steps from 0 to beta_max
    n_steps: int = 10
    sweeps_per_step: int = 1
    random_seed: Optional[int] = None
    # build-specific (as ParallelTemperingConfig)
    coupling_storage: str = "auto"
    field_cache: str = "auto"
    fixed_point_fields: bool = False
    row_shared_grid: bool = False
    row_shared_fields: int = 2
    site_order: str = "random"
    sequential_window: int = 1024
    device_index: Optional[int] = None
    autotune: Optional[bool] = None

    def __post_init__(self):
        self.check()

    def check(self):
        for name in ("population_size", "n_populations"):
            v = getattr(self, name)
            if int(v) != v or v < 1:
                raise ConfigurationError(f"{name} must be a positive integer")
        if self.population_size > MAX_POPULATION:
            raise ConfigurationError("population_size must not exceed 2^23 (use n_populations for more replicas)")
        if int(self.sweeps_per_step) != self.sweeps_per_step or self.sweeps_per_step < 1:
            raise ConfigurationError("sweeps_per_step must be a positive integer")
        if self.site_order not in ("random", "sequential"):
            raise ConfigurationError("site_order must be 'random' or 'sequential'")
        self.schedule()

    def schedule(self) -> np.ndarray:
        """float64 [steps + 1]: the inverse temperatures, the first 0."""
        if self.betas is None:
            if int(self.n_steps) != self.n_steps or self.n_steps < 1:
                raise ConfigurationError("n_steps must be a positive integer")
            if not np.isfinite(self.beta_max) or self.beta_max <= 0:
                raise ConfigurationError("beta_max must be positive and finite")
            return float(self.beta_max) * np.arange(int(self.n_steps) + 1, dtype=np.float64) / float(self.n_steps)
        b = np.asarray(self.betas, np.float64)
        if b.ndim != 1 or b.size < 2:
            raise ConfigurationError("betas must hold at least two inverse temperatures")
        if not np.all(np.isfinite(b)) or np.any(b < 0):
            raise ConfigurationError("betas must be finite and not negative")
        if b[0] != 0:
            raise ConfigurationError("betas must start at 0 (the run starts from random spins)")
        if np.any(b[1:] == 0):
            raise ConfigurationError("only the first of betas may be 0 (a sweep needs a finite temperature)")
        return b


class PopulationAnnealing:
    def __init__(self, config: PopulationAnnealingConfig):
        config.check()
        self.config = config
        self.betas = config.schedule()
        P = int(config.n_populations)
        self.log_partition = np.zeros(P)      # ln Z(betas[-1]) per population: n ln 2 + sum of the steps' ln Q
        self.free_energy = np.zeros(P)        # -log_partition / betas[-1]
        self.family_counts = np.zeros(P, np.int64)  # initial replicas with a descendant in the final population
        self.rho_t = np.zeros(P)              # N sum_i f_i^2, f_i the fraction of the population in family i
        self.survivor_fraction = np.zeros((len(self.betas) - 1, P))  # per step: slots whose replica kept its slot
        self.parents_history = None           # run(record_parents=True): int32 [steps, R]
        self.final_energies = None
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.use_cuda = self.device.type == "cuda"

    def run(self, model: IsingModel, update_rule: UpdateRule = UpdateRule.METROPOLIS, record_parents: bool = False) -> AnnealingResult:
        rule = rule_code(update_rule)
        cfg = self.config
        cfg.check()
        betas = self.betas = cfg.schedule()
        steps = len(betas) - 1
        Np, P, n = int(cfg.population_size), int(cfg.n_populations), model.n_spins
        R = Np * P
        site_mode = N.SITE_RANDOM if cfg.site_order == "random" else N.SITE_SEQUENTIAL
        dev_idx = cfg.device_index if cfg.device_index is not None else _device_index(model.device)
        t_start = time.time()
        log_z = np.full(P, n * np.log(2.0))
        family = np.tile(np.arange(Np, dtype=np.int64), P)  # the initial member every replica descends from, per population
        own = np.arange(R, dtype=np.int32)
        self.survivor_fraction = np.zeros((steps, P))
        history = np.zeros((steps, R), np.int32) if record_parents else None
        energy_history, temp_history, acc_history = [], [], []
        with AnnealEngine(dev_idx) as eng:
            eng.set_field_cache(cfg.field_cache)  # (before the couplings: "on" keeps a sparse matrix dense)
            if cfg.fixed_point_fields:
                eng.set_option("clf_fixed_point", 1)
            if cfg.row_shared_grid:
                eng.set_option("row_shared_grid", 1)
            if cfg.row_shared_fields != 2:
                eng.set_option("row_shared_fields", cfg.row_shared_fields)
            if cfg.site_order == "sequential":
                eng.set_sequential_windows(cfg.sequential_window)
            model.load_into(eng, storage=cfg.coupling_storage)
            eng.set_update_rule(rule)
            eng.init_replicas(R, seed=fresh_seed(cfg.random_seed))
            eng.set_temperatures(np.inf)  # beta = 0: the random spins are the equilibrium population
            eng.maybe_autotune(steps * int(cfg.sweeps_per_step), cfg.autotune)
            acc_prev = np.zeros(R, np.int64)
            for step in range(steps):
                parents, log_q = eng.resample(betas[step + 1] - betas[step], n_populations=P, round=step)
                eng.set_temperatures(1.0 / betas[step + 1])
                eng.sweep(int(cfg.sweeps_per_step), site_mode=site_mode)
                log_z = log_z + log_q
                family = family[parents]
                self.survivor_fraction[step] = (parents == own).reshape(P, Np).mean(axis=1)
                if history is not None:
                    history[step] = parents
                en, acc, _ = eng.snapshot(slots=False)
                energy_history.append(float(en[:Np].mean()))
                temp_history.append(float(1.0 / betas[step + 1]))
                acc_history.append(float((acc - acc_prev).sum()) / float(R * n * int(cfg.sweeps_per_step)))
                acc_prev = acc
            self.final_energies = eng.energies()
            best_energy, best_configuration, _ = eng.best()
        self.parents_history = history
        self.log_partition = log_z
        self.free_energy = -log_z / betas[-1]
        fam = family.reshape(P, Np)
        self.family_counts = np.asarray([np.unique(f).size for f in fam], np.int64)
        self.rho_t = np.asarray([Np * float(np.sum((np.bincount(f, minlength=Np) / Np) ** 2)) for f in fam])
        return AnnealingResult(
            best_configuration=torch.from_numpy(best_configuration.astype(np.float32)), best_energy=float(best_energy),
            energy_history=energy_history, temperature_history=temp_history, acceptance_rate_history=acc_history,
            total_time=time.time() - t_start, n_sweeps=steps * int(cfg.sweeps_per_step), algorithm="population_annealing",
            device=f"cuda:{dev_idx}", random_seed=cfg.random_seed)

    def __repr__(self) -> str:
        c = self.config
        return (f"PopulationAnnealing(population_size={c.population_size}, n_populations={c.n_populations}, "
                f"beta_max={self.betas[-1]:.3f}, steps={len(self.betas) - 1})")
