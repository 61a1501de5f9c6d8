"""ParallelTempering: replica exchange Monte Carlo with every replica resident on the GPU.

Host loop of the reference's spin_glass_rl/annealing/parallel_tempering.py:16-313: geometric /
linear / exponential ladder with index 0 the hottest, one Metropolis sweep of every replica per
step, nearest-neighbour exchanges every `exchange_interval` sweeps (skipping sweep 0) with a
random even/odd start, statistics and best-over-replicas on record sweeps only.  All replicas
advance in one kernel call between two events; an exchange swaps temperature labels on the
device instead of moving spin tensors (same Markov chain, no copies).

`exchange_method="all_pairs"` follows the reference's CPU branch (:222-232: every pair i < j behind the
gate `np.random.rand() < 0.1`, the criterion of `_attempt_single_exchange`, :234-258; pinned to the
fixture pt_allpairs_n16_r5).  On a CUDA device the reference routes the same setting through
`_cuda_optimized_exchange` instead (:222-226 -> :260-293: sequential ADJACENT pairs, fp32 probability with
the inverted sign, spin rows and energies swapped) -- a different exchange rule under the same name.  That
rule is available here as the stateless operator `CUDAKernelManager.parallel_tempering_exchange_optimized`
/ `sga_op_pt_exchange` (pinned to operator_n48), not through this class: `ParallelTempering` means the
CPU branch on every device.
"""
import time
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _native as N
from .engine import AnnealEngine
from .exceptions import AnnealingError, ConfigurationError
from .gpu_annealer import fresh_seed
from .ising_model import IsingModel, _device_index
from .result import AnnealingResult
from .spin_dynamics import UpdateRule, rule_code
from .temperature_scheduler import temperature_ladder


@dataclass
class ParallelTemperingConfig:
    n_replicas: int = 8
    n_sweeps: int = 1000
    temp_min: float = 0.1
    temp_max: float = 10.0
    temp_distribution: str = "geometric"
    exchange_interval: int = 10
    exchange_method: str = "nearest_neighbor"
    n_threads: Optional[int] = None  # accepted for compatibility; replicas run on the GPU
    record_interval: int = 10
    random_seed: Optional[int] = None
    # build-specific
    coupling_storage: str = "auto"
    field_cache: str = "auto"             # resident local fields where the problem allows (identical chain)
    fixed_point_fields: bool = False      # ... real-valued sparse and dense couplings too (option "clf_fixed_point")
    row_shared_grid: bool = False         # option "row_shared_grid": row-shared windows for dense J on a binary grid 2^-k
    #                                       under any h (same chain); acts with field_cache="off", where autotune picks the
    #                                       form or option "row_shared" = 1 forces it, under the Metropolis, Glauber and
    #                                       heat-bath rules (the autotuner's pick is the rule's it was timed under)
    row_shared_fields: int = 2            # option "row_shared_fields": the fields kernel of those windows over resident
    #                                       bit-planes -- 0 per proposed site, 1 per tile of sites wherever it can run, 2 where
    #                                       it was measured to win (same chain)
    site_order: str = "random"            # "random" | "sequential": typewriter sweeps, site t at update t (SITE_SEQUENTIAL)
    sequential_window: int = 1024         # sequential order: W of the sequential windows (set_sequential_windows; 0 = off) --
    #                                       one read of each coupling row per sweep for all replicas (same chain).  The form
    #                                       acts with field_cache="off"; under "auto" / "on" the cached-field kernels serve
    #                                       sequential sweeps as before
    device_index: Optional[int] = None
    autotune: Optional[bool] = None       # measured launch geometry (None: for long runs only)
    n_copies: int = 1                     # identical ladders run side by side (n_copies * n_replicas engine replicas), each
    #                                       exchanged on its own; histories and exchange statistics are copy 0's, the best is
    #                                       taken over all copies
    cluster_moves: bool = False           # isoenergetic cluster moves between copies 2c and 2c + 1 at equal slots after every
    #                                       exchange round (AnnealEngine.cluster_move_ladders; sparse couplings, an even n_copies)
    cluster_temp_max: Optional[float] = None  # ... only in the slots whose temperature is at or below this (None: all)
    measure_overlaps: bool = False        # histogram, per temperature, the spin overlap and (sparse couplings) the link overlap
    #                                       between copies 2c and 2c + 1 on the device (AnnealEngine.accumulate_ladder_overlaps;
    #                                       an even n_copies), after the exchange round and its cluster moves; read once at the
    #                                       end into ParallelTempering.overlap_statistics.  Off: the run issues no such call
    measure_after: int = 0                # ... only in exchange rounds with at least this many sweeps behind them
    measure_interval: int = 1             # ... in every measure_interval-th of those rounds, the first one included
    overlap_bins: Optional[int] = None    # ... None: exact, a bin per value (n + 1, links + 1); else the smallest power-of-two
    #                                       bin width that needs at most this many bins
    measure_class_overlaps: bool = False  # sum, per temperature, the overlap between copies 2c and 2c + 1 resolved by the classes
    #                                       of overlap_classes and its second moments on the device
    #                                       (AnnealEngine.accumulate_ladder_class_overlaps; an even n_copies), in the rounds
    #                                       measure_overlaps would measure (measure_after, measure_interval); read once at the end
    #                                       into ParallelTempering.class_overlap_statistics.  Off: the run issues no such call
    overlap_classes: Optional[np.ndarray] = None  # ... the class maps, int [n_maps, n] or [n] (encoders.lattice_planes for the
    #                                       planes of a lattice); a negative value puts a site in no class

    def __post_init__(self):
        if self.site_order not in ("random", "sequential"):
            raise ConfigurationError("site_order must be 'random' or 'sequential'")
        self.check_copies()

    def check_copies(self):
        if int(self.n_copies) != self.n_copies or self.n_copies < 1:
            raise ConfigurationError("n_copies must be a positive integer")
        if self.cluster_moves and (self.n_copies < 2 or self.n_copies % 2 != 0):
            raise ConfigurationError("cluster_moves needs an even n_copies >= 2 (the moves act between two copies of the ladder)")
        if self.n_copies > 1 and self.exchange_method == "all_pairs":
            raise ConfigurationError('n_copies > 1 is not implemented for exchange_method="all_pairs"')
        if self.measure_overlaps and (self.n_copies < 2 or self.n_copies % 2 != 0):
            raise ConfigurationError("measure_overlaps needs an even n_copies >= 2 (the overlaps are taken between two copies of the ladder)")
        if int(self.measure_after) != self.measure_after or self.measure_after < 0:
            raise ConfigurationError("measure_after must be a non-negative number of sweeps")
        if int(self.measure_interval) != self.measure_interval or self.measure_interval < 1:
            raise ConfigurationError("measure_interval must be a positive number of exchange rounds")
        if self.overlap_bins is not None and (int(self.overlap_bins) != self.overlap_bins or self.overlap_bins < 1):
            raise ConfigurationError("overlap_bins must be None or a positive integer")
        if self.measure_class_overlaps:
            if self.n_copies < 2 or self.n_copies % 2 != 0:
                raise ConfigurationError("measure_class_overlaps needs an even n_copies >= 2 (the overlaps are taken between two copies of the ladder)")
            if self.overlap_classes is None:
                raise ConfigurationError("measure_class_overlaps needs overlap_classes, the class maps [n_maps, n]")
            cl = np.asarray(self.overlap_classes)
            if cl.ndim not in (1, 2) or cl.size == 0 or not np.issubdtype(cl.dtype, np.integer):
                raise ConfigurationError("overlap_classes must be an integer array [n_maps, n] or [n]")
            if cl.max() < 0:
                raise ConfigurationError("overlap_classes puts no site in any class")
            if cl.max() >= 2 ** 31 or cl.min() < -2 ** 31:
                raise ConfigurationError("overlap_classes must hold 32-bit values")


def bin_shift(largest: int, max_bins: Optional[int]) -> int:
    """The smallest shift s in [0, 31] with (largest >> s) + 1 <= max_bins (None: 0, a bin per value); 31 where none is
    (the last bin then takes the rest: the engine clamps)."""
    if max_bins is None:
        return 0
    return next((s for s in range(32) if (int(largest) >> s) + 1 <= max_bins), 31)


@dataclass
class OverlapStatistics:
    """Histograms of the overlaps between two copies of a ladder, per temperature, as accumulate_ladder_overlaps left them:
    hist_q[c, s, k] counts the measurements of copy pair c at temperatures[s] whose distance d (differing sites; q = 1 -
    2 d / n) fell into bin k = min(d >> q_shift, bins - 1); hist_l the same for the broken links b (q_l = 1 - 2 b /
    n_links), None where the couplings are not sparse.  Everything here is plain numpy on the host."""
    temperatures: np.ndarray
    n: int
    n_links: Optional[int]
    hist_q: np.ndarray
    q_shift: int = 0
    hist_l: Optional[np.ndarray] = None
    l_shift: int = 0

    @staticmethod
    def _centres(bins: int, shift: int, largest: int) -> np.ndarray:
        """1 - 2 c_k / largest, c_k the middle of the values bin k holds: [k << shift, (k + 1) << shift) cut at `largest`,
        the last bin up to `largest` (the clamp)."""
        k = np.arange(bins, dtype=np.float64)
        lo = np.minimum(k * 2.0 ** shift, float(largest))
        hi = np.minimum((k + 1.0) * 2.0 ** shift - 1.0, float(largest))
        hi[-1] = max(float(largest), lo[-1])
        return 1.0 - (lo + hi) / max(float(largest), 1.0)

    def q_values(self) -> np.ndarray:
        """The overlap q at the centre of every bin of hist_q (exact where q_shift == 0)."""
        return self._centres(self.hist_q.shape[-1], self.q_shift, self.n)

    def link_values(self) -> np.ndarray:
        """The link overlap q_l at the centre of every bin of hist_l."""
        if self.hist_l is None:
            raise ConfigurationError("no link overlaps were measured (the couplings are not sparse)")
        return self._centres(self.hist_l.shape[-1], self.l_shift, self.n_links)

    @staticmethod
    def _mean(hist, values) -> np.ndarray:
        w = np.asarray(hist, np.float64).sum(axis=0)  # over the copy pairs: [slots, bins]
        total = w.sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            return (w * values).sum(axis=1) / total

    def moments(self):
        """(<q^2>, <q^4>) per temperature, over all copy pairs (NaN where nothing was measured)."""
        q = self.q_values()
        return self._mean(self.hist_q, q ** 2), self._mean(self.hist_q, q ** 4)

    def binder(self) -> np.ndarray:
        """The Binder ratio (3 - <q^4> / <q^2>^2) / 2 per temperature."""
        q2, q4 = self.moments()
        with np.errstate(divide="ignore", invalid="ignore"):
            return 0.5 * (3.0 - q4 / q2 ** 2)

    def link_overlap(self) -> np.ndarray:
        """<q_l> per temperature, over all copy pairs."""
        return self._mean(self.hist_l, self.link_values())


@dataclass
class ClassOverlapStatistics:
    """First and second moments of the class-resolved overlaps between two copies of a ladder, per temperature, as
    accumulate_ladder_class_overlaps left them.  For copy pair p, temperatures[s] and class map m, with D_c the sites of
    class c where the two copies differ (the class overlap is Q_c = N_c - 2 D_c): sum1[p, s, m, c] is the sum of D_c over
    the measurements, sum2[p, s, m, c, c'] the sum of D_c D_c' (None where it was not taken).  class_sizes[m, c] = N_c.
    Everything here is plain numpy on the host.

    susceptibility(k) and correlation_length() read the class index as a coordinate: they are meaningful only where the
    classes are the planes of a periodic lattice (encoders.lattice_planes), every map one axis."""
    temperatures: np.ndarray
    class_sizes: np.ndarray
    measurements: int
    sum1: np.ndarray
    sum2: Optional[np.ndarray] = None

    def class_correlations(self) -> np.ndarray:
        """<Q_c Q_c'> per copy pair, temperature and map, float64 [pairs, slots, n_maps, C, C], from
        N_c N_c' - 2 N_c <D_c'> - 2 N_c' <D_c> + 4 <D_c D_c'>: formed in exact integers as T N_c N_c' - 2 N_c S1_c' -
        2 N_c' S1_c + 4 S2_cc' (T measurements) before the one division by T.  NaN where nothing was measured."""
        if self.sum2 is None:
            raise ConfigurationError("no second moments were measured (sum2 is None)")
        T = int(self.measurements)
        N_ = [[int(v) for v in row] for row in np.asarray(self.class_sizes)]
        s1, s2 = np.asarray(self.sum1), np.asarray(self.sum2)
        out = np.full(s2.shape, np.nan, np.float64)
        if T <= 0:
            return out
        for idx in np.ndindex(*s2.shape[:3]):
            Nm = np.asarray(N_[idx[2]], dtype=object)
            a = np.asarray([int(v) for v in s1[idx]], dtype=object)
            b = np.asarray([[int(v) for v in row] for row in s2[idx]], dtype=object)
            num = T * np.outer(Nm, Nm) - 2 * np.outer(Nm, a) - 2 * np.outer(a, Nm) + 4 * b  # Python integers: exact
            out[idx] = (num / T).astype(np.float64)
        return out

    def susceptibility(self, k: float) -> np.ndarray:
        """chi(k) = (1 / n) sum_{c, c'} <Q_c Q_c'> cos(k (c - c')) per temperature, averaged over the maps and the copy
        pairs; n = the sites of a map, sum_c N_c."""
        qq = self.class_correlations()
        c = np.arange(qq.shape[-1], dtype=np.float64)
        w = np.cos(float(k) * (c[:, None] - c[None, :]))
        n_sites = np.asarray(self.class_sizes, np.float64).sum(axis=1)  # [n_maps]
        chi = (qq * w).sum(axis=(3, 4)) / n_sites[None, None, :]
        return chi.mean(axis=(0, 2))

    def correlation_length(self) -> np.ndarray:
        """xi = sqrt(chi(0) / chi(k_min) - 1) / (2 sin(k_min / 2)) per temperature, k_min = 2 pi / C: the finite-size
        correlation length whose ratio xi / L crosses at T_c.  NaN where nothing was measured or the radicand is negative
        or undefined (chi(k_min) = chi(0) = 0); +inf where chi(k_min) = 0 < chi(0), zero meaning |chi(k_min)| <= 1e-12 chi(0).  Meaningful only where the
        classes are the planes of a periodic lattice."""
        C = self.sum1.shape[-1]
        k_min = 2.0 * np.pi / C
        chi0, chik = self.susceptibility(0.0), self.susceptibility(k_min)
        zero = np.abs(chik) <= 1e-12 * np.abs(chi0)  # chi(k_min) = 0 up to the rounding of the cosine sum
        with np.errstate(divide="ignore", invalid="ignore"):
            rad = np.where(zero, np.where(chi0 > 0, np.inf, np.nan), chi0 / np.where(zero, 1.0, chik) - 1.0)
            return np.sqrt(np.where(rad >= 0, rad, np.nan)) / (2.0 * np.sin(k_min / 2.0))


def planned_measurements(n_sweeps: int, exchange_interval: int, measure_after: int, measure_interval: int) -> int:
    """The exchange rounds a run measures in: those behind sweeps s = exchange_interval, 2 exchange_interval ... < n_sweeps
    with s + 1 >= measure_after, every measure_interval-th of them, the first one included."""
    last = (n_sweeps - 1) // exchange_interval                       # s = k exchange_interval, 1 <= k <= last
    first = max(1, -(-(measure_after - 1) // exchange_interval))      # ... and k exchange_interval + 1 >= measure_after
    eligible = max(0, last - first + 1)
    return -(-eligible // measure_interval)


def class_sizes(classes: np.ndarray, n_classes: int) -> np.ndarray:
    """N[m, c]: the sites of class c in map m (values outside [0, n_classes) are no class), int64 [n_maps, n_classes]."""
    cl = np.asarray(classes)
    cl = cl.reshape(1, -1) if cl.ndim == 1 else cl
    return np.stack([np.bincount(row[(row >= 0) & (row < n_classes)], minlength=n_classes) for row in cl]).astype(np.int64)


class ParallelTempering:
    def __init__(self, config: ParallelTemperingConfig):
        if config.n_replicas < 2:
            raise ConfigurationError("parallel tempering needs at least 2 replicas")
        if config.exchange_interval <= 0 or config.record_interval <= 0 or config.n_sweeps <= 0:
            raise ConfigurationError("intervals and n_sweeps must be positive")
        config.check_copies()
        self.config = config
        self.temperatures = temperature_ladder(config.n_replicas, config.temp_min,
                                               config.temp_max, config.temp_distribution)
        R = config.n_replicas
        self.exchange_attempts = np.zeros((R - 1,))
        self.exchange_accepts = np.zeros((R - 1,))
        self.energy_histories: List[List[float]] = [[] for _ in range(R)]
        self.temp_histories: List[List[float]] = [[] for _ in range(R)]
        self.slot_acceptance = np.zeros(R)
        # isoenergetic cluster moves of the last run(): moves made, those that flipped anything, sites flipped, largest cluster
        self.cluster_moves_made = self.cluster_moves_flipped = self.cluster_sites_flipped = self.cluster_size_max = 0
        # measure_overlaps: the histograms of the last run() (OverlapStatistics) and the exchange rounds that were measured
        self.overlap_statistics: Optional[OverlapStatistics] = None
        self.overlap_rounds_measured = 0
        # measure_class_overlaps: the sums of the last run() (ClassOverlapStatistics)
        self.class_overlap_statistics: Optional[ClassOverlapStatistics] = None
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.use_cuda = self.device.type == "cuda"

    def run(self, model: IsingModel, update_rule: UpdateRule = UpdateRule.METROPOLIS,
            _replay=None) -> AnnealingResult:
        """`_replay`: parity-test hook, dict(s0, site[ns,R,n], u[ns,R,n], exch_start, exch_u)
        recorded from the reference, replacing every Philox draw."""
        rule = rule_code(update_rule)
        cfg = self.config
        cfg.check_copies()
        if cfg.exchange_method not in ("nearest_neighbor", "all_pairs"):
            raise ValueError(f"Unknown exchange method: {cfg.exchange_method}")  # reference :212
        all_pairs = cfg.exchange_method == "all_pairs"
        site_mode = N.SITE_RANDOM if cfg.site_order == "random" else N.SITE_SEQUENTIAL  # (the _replay hook: SITE_REPLAY)
        # all_pairs: the gate `np.random.rand() < 0.1` of the reference (:222-232) only selects which
        # pairs are attempted; it is drawn on the host (seeded), the attempts run on the engine
        gate_rng = np.random.RandomState(fresh_seed(cfg.random_seed) & 0x7FFFFFFF)
        pair_list = [(i, j) for i in range(cfg.n_replicas - 1) for j in range(i + 1, cfg.n_replicas)]
        t_start = time.time()
        R, n, C = cfg.n_replicas, model.n_spins, int(cfg.n_copies)
        temps = np.asarray(self.temperatures, np.float64)
        self.class_overlap_statistics = None
        class_plan = self.class_overlap_plan(n) if cfg.measure_class_overlaps else None  # (refused before the device is touched)
        if C > 1 and _replay is not None:
            raise ConfigurationError("the replay hook drives one ladder (n_copies = 1)")
        # the slots the cluster moves act in: the ladder is monotone (index 0 the hottest), so they are one range
        cl_lo, cl_hi = 0, R
        if cfg.cluster_moves and cfg.cluster_temp_max is not None:
            cold = np.nonzero(temps <= cfg.cluster_temp_max)[0]
            cl_lo, cl_hi = (int(cold.min()), int(cold.max()) + 1) if cold.size else (0, 0)
        self.cluster_moves_made = self.cluster_moves_flipped = self.cluster_sites_flipped = self.cluster_size_max = 0
        dev_idx = cfg.device_index if cfg.device_index is not None else _device_index(model.device)
        best_energy, best_configuration = float("inf"), None
        acc_slot, att_slot = np.zeros(R, np.int64), np.zeros(R, np.int64)
        with AnnealEngine(dev_idx) as eng:
            eng.set_field_cache(cfg.field_cache)  # (before the couplings: "on" keeps a sparse matrix dense)
            if cfg.fixed_point_fields:
                eng.set_option("clf_fixed_point", 1)  # (read when the couplings are set)
            if cfg.row_shared_grid:
                eng.set_option("row_shared_grid", 1)  # (read at every sweep; acts with field_cache="off")
            if cfg.row_shared_fields != 2:
                eng.set_option("row_shared_fields", cfg.row_shared_fields)  # (read at every sweep)
            if cfg.site_order == "sequential":
                eng.set_sequential_windows(cfg.sequential_window)  # (read at every sweep; acts with field_cache="off")
            model.load_into(eng, storage=cfg.coupling_storage)
            eng.set_update_rule(rule)
            eng.init_replicas(C * R, seed=fresh_seed(cfg.random_seed),
                              s0=None if _replay is None else _replay["s0"])
            eng.set_ladder(np.tile(temps, C) if C > 1 else temps, C)
            if cfg.cluster_moves:  # an empty range moves nothing: what the engine refuses, it refuses here
                try:
                    eng.cluster_move_ladders(0, 0, round=0, sizes=False)
                except AnnealingError as exc:
                    raise ConfigurationError(f"cluster_moves: {exc.message}") from exc
            hist_q = hist_l = None
            self.overlap_statistics, self.overlap_rounds_measured, eligible = None, 0, 0
            if cfg.measure_overlaps:  # the histograms stay on the device for the whole run
                try:
                    n_links = eng.link_count()
                except AnnealingError as exc:  # dense and implicit couplings: the spin part only
                    if exc.details.get("code") != N.ERR_UNSUPPORTED:
                        raise
                    n_links = None
                q_shift = bin_shift(n, cfg.overlap_bins)
                hdev = torch.device("cuda", dev_idx)
                hist_q = torch.zeros((C // 2, R, (n >> q_shift) + 1), dtype=torch.int64, device=hdev)
                l_shift = 0
                if n_links is not None:
                    l_shift = bin_shift(n_links, cfg.overlap_bins)
                    hist_l = torch.zeros((C // 2, R, min((n_links >> l_shift) + 1, cfg.overlap_bins or n_links + 1)),
                                         dtype=torch.int64, device=hdev)
            cls_map = cls_sum1 = cls_sum2 = None
            cls_measured = 0
            if class_plan is not None:  # the map and the sums stay on the device for the whole run
                cdev = torch.device("cuda", dev_idx)
                cls_map = torch.from_numpy(class_plan[0]).to(cdev)
                cls_sum1 = torch.zeros((C // 2, R) + class_plan[0].shape[:1] + (class_plan[1],), dtype=torch.int64, device=cdev)
                cls_sum2 = torch.zeros(tuple(cls_sum1.shape) + (class_plan[1],), dtype=torch.int64, device=cdev)
            eng.maybe_autotune(cfg.n_sweeps, cfg.autotune)
            slot_to_rep = np.arange(R, dtype=np.int32)
            acc_prev = np.zeros(R, np.int64)
            rnd = ucur = 0
            sweep = 0
            while sweep < cfg.n_sweeps:
                # advance to the next sweep index that carries an event
                stop = sweep
                while stop < cfg.n_sweeps - 1 and not self._event(stop):
                    stop += 1
                count = stop - sweep + 1
                if _replay is None:
                    eng.sweep(count, site_mode=site_mode)
                else:
                    inv = np.argsort(slot_to_rep)
                    site = _replay["site"][sweep:stop + 1][:, inv].transpose(1, 0, 2).reshape(R, -1)
                    u = _replay["u"][sweep:stop + 1][:, inv].transpose(1, 0, 2).reshape(R, -1)
                    eng.sweep(count, site_mode=N.SITE_REPLAY, replay_site=site, replay_u=u)
                exchange_now = stop % cfg.exchange_interval == 0 and stop > 0  # reference :113
                if exchange_now and all_pairs:
                    if _replay is None:
                        gates = gate_rng.rand(len(pair_list)) < 0.1
                        eng.exchange_pairs([p for p, g in zip(pair_list, gates) if g])
                    else:  # the recorded stream: a gate draw per pair, an exchange draw behind an open gate
                        stream, chosen, uu = _replay["np_rand_all"], [], []
                        for p in pair_list:
                            g = stream[ucur]
                            ucur += 1
                            if g < 0.1:
                                chosen.append(p)
                                uu.append(stream[ucur])
                                ucur += 1
                        eng.exchange_pairs(chosen, u=np.asarray(uu, np.float64))
                    rnd += 1
                elif exchange_now:
                    if _replay is None:
                        eng.exchange(count=False)  # enqueued behind the sweeps, no host round trip
                    else:
                        start = int(_replay["exch_start"][rnd])
                        npairs = len(range(start, R - 1, 2))
                        uu = np.zeros(R // 2)
                        uu[:npairs] = _replay["exch_u"][ucur:ucur + npairs]
                        eng.exchange(start=[start], u=uu, count=False)
                        ucur += npairs
                    rnd += 1
                if exchange_now and cfg.cluster_moves and cl_hi > cl_lo:
                    # round: the engine's exchange-round counter, just advanced by the exchange
                    sz = eng.cluster_move_ladders(cl_lo, cl_hi)
                    self.cluster_moves_made += int(sz.size)
                    self.cluster_moves_flipped += int(np.count_nonzero(sz))
                    self.cluster_sites_flipped += int(sz.sum())
                    self.cluster_size_max = max(self.cluster_size_max, int(sz.max()))
                if exchange_now and hist_q is not None and stop + 1 >= cfg.measure_after:
                    if eligible % cfg.measure_interval == 0:
                        eng.accumulate_ladder_overlaps(hist_q, hist_l, q_shift=q_shift, l_shift=l_shift)
                        self.overlap_rounds_measured += 1
                    eligible += 1
                if exchange_now and cls_map is not None and stop + 1 >= cfg.measure_after:
                    if cls_measured % cfg.measure_interval == 0:
                        eng.accumulate_ladder_class_overlaps(cls_map, class_plan[1], cls_sum1, cls_sum2)
                    cls_measured += 1
                # one synchronisation per event: energies (an exchange moves labels, not energies),
                # acceptance counters, ladder permutation
                en_rep, acc_now, full_map = eng.snapshot()
                acc_now, new_map = acc_now[:R], full_map[:R]  # copy 0: ladder 0 holds replicas 0 ... R - 1
                # per-slot acceptance bookkeeping (the reference's SpinDynamics stay with slots):
                # these sweeps ran under the permutation in force BEFORE the exchange
                acc_slot += (acc_now - acc_prev)[slot_to_rep]
                att_slot += count * n
                acc_prev = acc_now
                slot_to_rep = new_map
                if stop % cfg.record_interval == 0:  # reference :117-125
                    en = en_rep[slot_to_rep]
                    for i in range(R):
                        self.energy_histories[i].append(float(en[i]))
                        self.temp_histories[i].append(float(temps[i]))
                    if C > 1:  # the best over all copies
                        en = en_rep[full_map]
                    i_best = int(np.argmin(en))
                    if en[i_best] < best_energy:
                        best_energy = float(en[i_best])
                        best_configuration = eng.spins(int(full_map[i_best]))
                sweep = stop + 1
            att, acc = eng.exchange_stats()
            self.exchange_attempts = att[:R - 1].astype(np.float64)
            self.exchange_accepts = acc[:R - 1].astype(np.float64)
            self.final_spins = eng.spins()[slot_to_rep]
            # the final overlap matrix, formed where the spins are (sga_get_overlaps), in slot order like final_spins
            self._final_overlaps = eng.overlaps()[np.ix_(slot_to_rep, slot_to_rep)].astype(np.float64) / n
            if hist_q is not None:  # (the reads above waited for the engine's stream)
                self.overlap_statistics = OverlapStatistics(
                    temperatures=temps.copy(), n=int(n), n_links=n_links, hist_q=hist_q.cpu().numpy(), q_shift=q_shift,
                    hist_l=None if hist_l is None else hist_l.cpu().numpy(), l_shift=l_shift)
            if cls_map is not None:
                self.class_overlap_statistics = ClassOverlapStatistics(
                    temperatures=temps.copy(), class_sizes=class_plan[2], measurements=-(-cls_measured // cfg.measure_interval),
                    sum1=cls_sum1.cpu().numpy().view(np.uint64), sum2=cls_sum2.cpu().numpy().view(np.uint64))
        self.slot_acceptance = acc_slot / np.maximum(att_slot, 1)
        total_time = time.time() - t_start
        return AnnealingResult(
            best_configuration=torch.from_numpy(best_configuration.astype(np.float32)),
            best_energy=best_energy, energy_history=self.energy_histories[0],
            temperature_history=self.temp_histories[0],
            acceptance_rate_history=[float(x) for x in self.slot_acceptance],
            total_time=total_time, n_sweeps=cfg.n_sweeps, algorithm="parallel_tempering",
            device=f"cuda:{dev_idx}", random_seed=cfg.random_seed)

    def class_overlap_plan(self, n: int):
        """(class maps int32 [n_maps, n], n_classes, class sizes, planned measurements) of measure_class_overlaps for a
        model of n spins; ConfigurationError where the maps do not fit the model, or where the sums could overflow:
        measurements x max N_c^2 must stay below 2^63."""
        cfg = self.config
        cfg.check_copies()
        cl = np.asarray(cfg.overlap_classes)
        cl = np.ascontiguousarray(cl.reshape(1, -1) if cl.ndim == 1 else cl, dtype=np.int32)
        if cl.shape[1] != n:
            raise ConfigurationError(f"overlap_classes has {cl.shape[1]} sites, the model has {n}")
        n_classes = int(cl.max()) + 1
        sizes = class_sizes(cl, n_classes)
        planned = planned_measurements(cfg.n_sweeps, cfg.exchange_interval, cfg.measure_after, cfg.measure_interval)
        if planned * int(sizes.max()) ** 2 >= 2 ** 63:
            raise ConfigurationError(f"measure_class_overlaps: {planned} measurements of classes of up to {int(sizes.max())} sites "
                                     "could overflow the 64-bit sums (measurements x max N_c^2 must stay below 2^63)")
        return cl, n_classes, sizes, planned

    def _event(self, sweep: int) -> bool:
        c = self.config
        return (sweep % c.exchange_interval == 0 and sweep > 0) or sweep % c.record_interval == 0

    def replica_overlaps(self) -> np.ndarray:
        """q_ab = (1/n) sum_i s_i^a s_i^b of the final configurations as float64 [R, R], in slot (temperature) order:
        entry [i, j] relates the replicas that ended at temperatures[i] and temperatures[j].  After run()."""
        q = getattr(self, "_final_overlaps", None)
        if q is None:
            raise ConfigurationError("replica_overlaps() needs a finished run()")
        return q.copy()

    def get_exchange_rates(self) -> np.ndarray:
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(self.exchange_attempts > 0, self.exchange_accepts / self.exchange_attempts, 0.0)
        return r

    def get_statistics(self) -> Dict:
        rates = self.get_exchange_rates()
        finals = [h[-1] if h else float("inf") for h in self.energy_histories]
        return {"n_replicas": self.config.n_replicas, "temperatures": self.temperatures,
                "exchange_rates": rates.tolist(), "mean_exchange_rate": float(np.mean(rates)),
                "final_energies": finals, "best_energy": min(finals),
                "energy_range": max(finals) - min(finals),
                "total_exchanges_attempted": self.exchange_attempts.sum(),
                "total_exchanges_accepted": self.exchange_accepts.sum()}

    def __repr__(self) -> str:
        c = self.config
        return (f"ParallelTempering(n_replicas={c.n_replicas}, "
                f"temp_range=[{c.temp_min:.2f}, {c.temp_max:.2f}], n_sweeps={c.n_sweeps})")
