"""BatchProcessor: many independent Ising models through one engine.

Interface of the reference's spin_glass_rl/annealing/batch_processor.py:23-555
(`BatchConfig`, `BatchProcessor.process_models_batch / process_models_stream`): a list of
models goes in, one AnnealingResult per model comes out.  The reference loops a GPUAnnealer
over the models in a thread pool (:423-454).  Here models of equal size are stacked into ONE
engine (`sga_set_dense_batch`): every model gets `replicas_per_model` replicas, a single
kernel launch sweeps all of them (each replica reads its own model's coupling rows), and with
more than one replica per model each model is its own temperature ladder.  Models with sparse couplings
(`couplings.is_sparse`, the reference's default) of any sizes go, in input order and `batch_size` at a time, to
ONE engine kept as CSR (`sga_set_csr_batch`: one launch per sweep call, each replica on its own model's rows);
a chunk the ragged engine refuses (non-zero diagonal, asymmetric J) takes the stacked path.  Simulated
annealing semantics per replica are those of GPUAnnealer (schedule, best at sweep ends).

`GPUAnnealerConfig.field_cache` is handed to the engine before the couplings are set, as GPUAnnealer does.  A stacked
dense batch whose models all qualify (integer symmetric J, zero diagonal, h in multiples of 1/2) then keeps every
replica's local fields resident and reads a coupling row on accept only -- the same chain, so every result field
but `total_time` is the same for "on", "auto" and "off".  On the ragged (sparse) path "auto" and "off" stream; "on"
is refused by the ragged engine (SGA_ERR_UNSUPPORTED), which sends the chunk to the stacked path like any other
refusal.

`BatchConfig.ragged_field_cache=True` (build-specific, default False) sets the engine option "ragged_field_cache"
before the couplings: the ragged engine then serves `field_cache` "on" / "auto" itself -- every replica's local fields
of ITS model resident, one workgroup of 4 or 8 waves per replica, a row read on accept only; the same chain, so again
every result field but `total_time` is unchanged.  A chunk that does not qualify (a model with real-valued J, row sums
of 2^15 or more, duplicate entries, h off the half-integers) is refused under "on" and takes the stacked path; under
"auto" it streams on the ragged engine.

`annealer_config.fixed_point_fields=True` beside it sets the engine option "clf_fixed_point" as well: a chunk the
int16 form does not take (real-valued J such as distances, h off the half-integers, integer fields of 2^15 or more)
then runs the fixed-point form on the ragged engine -- D = 2^k J s as exact int32 | int64 at one batch-wide k; the
same chain once more.  Without `ragged_field_cache` the flag does nothing on the ragged path.

`BatchConfig.stacked_fixed_point=True` (build-specific, default False) together with
`annealer_config.fixed_point_fields=True` sets the engine options "clf_fixed_point" and "batch_fixed_point" before the
couplings of a STACKED batch: `field_cache` "on" / "auto" then also act on stacked batches the integer form does not
take -- real-valued J (half- and quarter-valued physical-convention encodings, binary-grid couplings, distances) or an
h off the half-integers.  The fields are D = 2^k J_m s as exact int32 | int64 at one batch-wide k, each replica on its
own model's rows; the same chain, so every result field but `total_time` equals the "off" result.  A batch that does
not qualify (f64-canonical J, an asymmetric J or a non-zero diagonal in some model) fails under "on" and runs the row
kernels under "auto".  With either flag unset the stacked path is what it was.

`BatchConfig.shared_couplings=True` (build-specific, default False): inside a chunk of dense models of one size, a run of
two or more CONSECUTIVE models that hold the same couplings (`shared_coupling_runs`: the same tensor object, the same
storage, or equal values) goes to ONE engine through `set_dense_shared` -- the matrix is handed over, packed and kept
once, each model contributes its field vector alone; what lies between two runs is stacked as before.  Such a run is
the same graph under many bias vectors: a policy's proposals, sub-problems with clamped variables, a field scan.  Every
segment is annealed as `process_models_batch` would anneal it on its own (replicas numbered from the segment's first
model), so a chunk that is one run gives the default path's results field for field but `total_time`.  All engine
options above act on a shared run as on a stacked batch.

The same switch acts on sparse chunks: a run of two or more CONSECUTIVE sparse models of one size whose coalesced COO
indices and values are equal (`shared_sparse_runs`: the same tensor object, the same storage, or equal content) goes to
ONE engine through `set_csr_shared` -- the entries are held once, and the several-updates-per-step and bit-spin CSR
forms, closed to ragged batches, serve it; what lies between two runs stays on `set_csr_batch`.  Every segment's
replicas keep the numbers they have in the chunk's one ragged engine (the segment's engine is a shard that starts at
the segment's first replica), so every result field but `total_time` is the default path's.  A segment an engine
refuses sends the whole chunk down the default path.
"""
import time
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional

import numpy as np
import torch

from .engine import AnnealEngine
from .exceptions import AnnealingError
from .gpu_annealer import GPUAnnealerConfig, fresh_seed
from . import _native as N
from .ising_model import IsingModel, coo_to_csr
from .result import AnnealingResult
from .temperature_scheduler import TemperatureScheduler


@dataclass
class BatchConfig:
    batch_size: int = 32
    max_memory_usage: float = 0.8
    prefetch_batches: int = 2
    use_mixed_precision: bool = False
    enable_gradient_checkpointing: bool = True
    memory_optimization_level: int = 1
    streaming_mode: bool = False
    checkpoint_interval: int = 100
    replicas_per_model: int = 1  # build-specific: independent restarts per model, best is kept
    ragged_field_cache: bool = False  # build-specific: sparse chunks serve field_cache "on" / "auto" on the ragged engine
    stacked_fixed_point: bool = False  # build-specific: stacked real-valued batches serve field_cache "on" / "auto" (fixed point)
    shared_couplings: bool = False  # build-specific: runs of models with one coupling matrix go through set_dense_shared / set_csr_shared

    def __post_init__(self):
        if self.batch_size <= 0:
            raise ValueError("Batch size must be positive")
        if not 0 < self.max_memory_usage <= 1:
            raise ValueError("Max memory usage must be between 0 and 1")
        if self.memory_optimization_level not in (0, 1, 2):
            raise ValueError("Memory optimization level must be 0, 1, or 2")
        if self.replicas_per_model <= 0:
            raise ValueError("replicas_per_model must be positive")
        if not isinstance(self.stacked_fixed_point, bool):
            raise ValueError("stacked_fixed_point must be a bool")
        if not isinstance(self.shared_couplings, bool):
            raise ValueError("shared_couplings must be a bool")


def _same_couplings(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a is b:
        return True
    if a.is_sparse or b.is_sparse or a.shape != b.shape:
        return False
    if a.dtype == b.dtype and a.device == b.device and a.data_ptr() == b.data_ptr() and a.stride() == b.stride():
        return True  # two views of one storage
    if a.device != b.device:
        a, b = a.detach().cpu(), b.detach().cpu()
    return a.dtype == b.dtype and bool(torch.equal(a, b))


def shared_coupling_runs(models) -> List[tuple]:
    """[(start, stop), ...]: the maximal runs models[start:stop] of two or more CONSECUTIVE dense models that share
    their couplings -- the same tensor object, or the same storage pointer, shape and strides, or else equal values
    (`torch.equal`).  A sparse model or a differing matrix ends a run; a run of one is not shared.  Pure: no engine,
    no GPU needed."""
    runs, start = [], 0
    while start < len(models):
        stop = start + 1
        first = models[start].couplings
        if not first.is_sparse:
            while stop < len(models) and _same_couplings(first, models[stop].couplings):
                stop += 1
        if stop - start >= 2:
            runs.append((start, stop))
        start = stop
    return runs


def _same_sparse_couplings(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a is b:
        return True
    if not (a.is_sparse and b.is_sparse) or a.shape != b.shape:
        return False
    a, b = a.coalesce(), b.coalesce()
    ia, ib, va, vb = a.indices(), b.indices(), a.values(), b.values()
    if ia.shape != ib.shape or va.dtype != vb.dtype:
        return False
    if ia.device == ib.device and ia.data_ptr() == ib.data_ptr() and va.data_ptr() == vb.data_ptr():
        return True  # one storage
    if ia.device != ib.device:
        ia, ib, va, vb = ia.cpu(), ib.cpu(), va.detach().cpu(), vb.detach().cpu()
    return bool(torch.equal(ia, ib)) and bool(torch.equal(va, vb))


def shared_sparse_runs(models) -> List[tuple]:
    """[(start, stop), ...]: the maximal runs models[start:stop] of two or more CONSECUTIVE sparse models of equal
    n_spins whose coalesced COO indices and values are equal -- the same tensor object, the same storage, or equal
    content.  A dense model, another size or a differing J ends a run; a run of one is not shared.  Pure: no engine, no
    GPU needed.  (`shared_coupling_runs` is the dense counterpart and keeps answering [] for sparse models.)"""
    runs, start = [], 0
    while start < len(models):
        stop = start + 1
        first = models[start]
        if first.couplings.is_sparse:
            while (stop < len(models) and models[stop].n_spins == first.n_spins and
                   _same_sparse_couplings(first.couplings, models[stop].couplings)):
                stop += 1
        if stop - start >= 2:
            runs.append((start, stop))
        start = stop
    return runs


class BatchProcessor:
    def __init__(self, annealer_config: GPUAnnealerConfig, batch_config: Optional[BatchConfig] = None,
                 device_index: int = 0):
        self.annealer_config = annealer_config
        self.batch_config = batch_config or BatchConfig()
        self.device_index = device_index
        self.processed_models = 0
        self.total_processing_time = 0.0
        self.batch_times: List[float] = []
        self.last_description: Optional[str] = None  # sga_describe of the last shared-coupling engine (shared_couplings)

    # ------------------------------------------------------------------ public API
    def process_models_batch(self, models: List[IsingModel]) -> List[AnnealingResult]:
        """Anneal every model; results come back in input order."""
        results: List[Optional[AnnealingResult]] = [None] * len(models)
        by_size: Dict[int, List[int]] = {}
        sparse: List[int] = []
        for i, m in enumerate(models):
            if m.couplings.is_sparse:
                sparse.append(i)
            else:
                by_size.setdefault(m.n_spins, []).append(i)
        bs = self.batch_config.batch_size
        for lo in range(0, len(sparse), bs):
            part = sparse[lo:lo + bs]
            t0 = time.time()
            out = self._anneal_sparse([models[i] for i in part])
            if out is None:  # refused by the ragged engine: the stacked path, by size
                for i in part:
                    by_size.setdefault(models[i].n_spins, []).append(i)
                continue
            for i, r in zip(part, out):
                results[i] = r
            self.batch_times.append(time.time() - t0)
        for _, idxs in sorted(by_size.items()):
            idxs = sorted(idxs)
            for lo in range(0, len(idxs), self.batch_config.batch_size):
                part = idxs[lo:lo + self.batch_config.batch_size]
                t0 = time.time()
                for i, r in zip(part, self._anneal_dense([models[i] for i in part])):
                    results[i] = r
                self.batch_times.append(time.time() - t0)
        self.processed_models += len(models)
        self.total_processing_time += sum(self.batch_times[-len(by_size):])
        return results  # type: ignore[return-value]

    def process_models_stream(self, models: Iterable[IsingModel]):
        """Generator form (reference :290-345): yields lists of results batch by batch."""
        chunk: List[IsingModel] = []
        for m in models:
            chunk.append(m)
            if len(chunk) == self.batch_config.batch_size:
                yield self.process_models_batch(chunk)
                chunk = []
        if chunk:
            yield self.process_models_batch(chunk)

    def get_processing_stats(self) -> Dict:
        n = max(len(self.batch_times), 1)
        return {"processed_models": self.processed_models,
                "total_processing_time": self.total_processing_time,
                "average_batch_time": float(np.mean(self.batch_times)) if self.batch_times else 0.0,
                "batches": len(self.batch_times),
                "models_per_second": self.processed_models / self.total_processing_time
                if self.total_processing_time > 0 else 0.0, "n": n}

    def reset(self) -> None:
        self.processed_models, self.total_processing_time, self.batch_times = 0, 0.0, []

    # ------------------------------------------------------------------ a chunk of dense models of one size
    def _anneal_dense(self, models: List[IsingModel]) -> List[AnnealingResult]:
        if not self.batch_config.shared_couplings:
            return self._anneal_stack(models)
        out: List[AnnealingResult] = []
        at = 0
        for start, stop in shared_coupling_runs(models) + [(len(models), len(models))]:
            if start > at:  # what lies before the run: stacked, as always
                out += self._anneal_stack(models[at:start])
            if stop > start:
                out += self._anneal_shared(models[start:stop])
            at = stop
        return out

    # ------------------------------------------------------------------ one run over one coupling matrix
    def _anneal_shared(self, models: List[IsingModel]) -> List[AnnealingResult]:
        J = models[0].dense_couplings().detach().cpu().numpy().astype(np.float32)
        H = np.stack([m.external_fields.detach().cpu().numpy().astype(np.float32) for m in models])
        s0 = np.stack([m.spins_int8() for m in models])  # [M, n]
        self.last_description = None

        def set_problem(eng):
            if self.batch_config.stacked_fixed_point and self.annealer_config.fixed_point_fields:
                eng.set_option("clf_fixed_point", 1)  # ([set] options: before the couplings)
                eng.set_option("batch_fixed_point", 1)
            eng.set_dense_shared(J, H, storage=self.annealer_config.coupling_storage)
            self.last_description = eng.describe()  # names the kind: "... shared-J models=M ..."

        return self._run(models, set_problem, s0)

    # ------------------------------------------------------------------ one stacked run
    def _anneal_stack(self, models: List[IsingModel]) -> List[AnnealingResult]:
        M, n = len(models), models[0].n_spins
        J = np.stack([m.dense_couplings().detach().cpu().numpy().astype(np.float32) for m in models])
        h = np.stack([m.external_fields.detach().cpu().numpy().astype(np.float32) for m in models])
        s0 = np.stack([m.spins_int8() for m in models])  # [M, n]
        def set_problem(eng):
            if self.batch_config.stacked_fixed_point and self.annealer_config.fixed_point_fields:
                eng.set_option("clf_fixed_point", 1)  # ([set] options: before the couplings)
                eng.set_option("batch_fixed_point", 1)
            eng.set_dense_batch(J, h, storage=self.annealer_config.coupling_storage)

        return self._run(models, set_problem, s0)

    # ------------------------------------------------------------------ a chunk of sparse models (any sizes)
    def _anneal_sparse(self, models: List[IsingModel]) -> Optional[List[AnnealingResult]]:
        runs = shared_sparse_runs(models) if self.batch_config.shared_couplings else []
        if not runs:
            return self._anneal_ragged(models)
        out: List[AnnealingResult] = []
        at = 0
        for start, stop in runs + [(len(models), len(models))]:
            seg = self._anneal_ragged(models[at:start], first=at) if start > at else []
            if seg is not None and stop > start:
                run = self._anneal_shared_csr(models[start:stop], first=start)
                seg = None if run is None else seg + run
            if seg is None:  # a segment refused: the chunk as the default path takes it
                return self._anneal_ragged(models)
            out += seg
            at = stop
        return out

    def _unsupported_is_none(self, call):
        try:
            return call()
        except AnnealingError as err:
            if (getattr(err, "details", None) or {}).get("code") == N.ERR_UNSUPPORTED:
                return None
            raise

    # ------------------------------------------------------------------ one run over one set of CSR rows
    def _anneal_shared_csr(self, models: List[IsingModel], first: int) -> Optional[List[AnnealingResult]]:
        """`first`: models of the chunk before this run.  The engine holds `first` all-zero field vectors in front of the
        run's and is initialised as the shard that starts at the run's first replica: replica numbers, and with them
        the random streams, are those of the chunk's one ragged engine.  (Zero fields change no batch-wide quantity.)"""
        rowptr, colidx, val = coo_to_csr(models[0].couplings)
        H = np.zeros((first + len(models), models[0].n_spins), np.float32)
        for i, m in enumerate(models):
            H[first + i] = m.external_fields.detach().cpu().numpy().astype(np.float32)
        s0 = np.stack([m.spins_int8() for m in models])  # [M, n]
        self.last_description = None

        def set_problem(eng):
            eng.set_csr_shared(rowptr, colidx, val, H)
            self.last_description = eng.describe()  # names the kind: "csr n=... shared-J models=M ..."

        return self._unsupported_is_none(lambda: self._run(models, set_problem, s0, first))

    # ------------------------------------------------------------------ one ragged run (sparse models, any sizes)
    def _anneal_ragged(self, models: List[IsingModel], first: int = 0) -> Optional[List[AnnealingResult]]:
        """None when the ragged engine refuses the chunk (SGA_ERR_UNSUPPORTED: diagonal / asymmetric J).
        `first` > 0 (a segment between two shared runs): that many one-spin models without couplings stand in front, and
        the engine is the shard behind them -- the segment's replicas keep their numbers in the chunk."""
        empty = (np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(1, np.float32))
        problems = [empty] * first + [coo_to_csr(m.couplings) + (m.external_fields.detach().cpu().numpy().astype(np.float32),)
                                      for m in models]
        n_max = max(m.n_spins for m in models)
        s0 = np.zeros((len(models), n_max), np.int8)  # [M, n_max], zero padded
        for i, m in enumerate(models):
            s0[i, :m.n_spins] = m.spins_int8()
        def set_problem(eng):
            if self.batch_config.ragged_field_cache:  # (a [set] option: before the couplings)
                eng.set_option("ragged_field_cache", 1)
                if self.annealer_config.fixed_point_fields:  # ([set] too: real-valued / wide chunks)
                    eng.set_option("clf_fixed_point", 1)
            eng.set_csr_batch(problems)

        return self._unsupported_is_none(lambda: self._run(models, set_problem, s0, first))

    def _run(self, models: List[IsingModel], set_problem, s0_models: np.ndarray, first: int = 0) -> List[AnnealingResult]:
        cfg, k = self.annealer_config, self.batch_config.replicas_per_model
        M = len(models)
        t0 = time.time()
        s0 = np.repeat(s0_models, k, axis=0)  # [M*k, n]
        schedule = TemperatureScheduler.create_schedule(
            cfg.schedule_type, cfg.initial_temp, cfg.final_temp, cfg.n_sweeps, **cfg.schedule_params)
        if cfg.schedule_type.value == "adaptive":
            raise AnnealingError("the adaptive schedule needs per-model feedback; use GPUAnnealer")
        temps = np.maximum(np.asarray([schedule.update(s) for s in range(cfg.n_sweeps)]), 1e-10)
        hist_e = [[] for _ in range(M)]
        with AnnealEngine(self.device_index) as eng:
            eng.set_field_cache(cfg.field_cache)  # (before the couplings, as GPUAnnealer.anneal)
            set_problem(eng)
            # (first > 0: the shard behind `first` models of the engine's batch, sparse segments only)
            shard = dict(R_global=(first + M) * k, replica0=first * k) if first else {}
            eng.init_replicas(M * k, seed=fresh_seed(cfg.random_seed), s0=s0, **shard)
            e0 = eng.energies().reshape(M, k).min(1)
            for m in range(M):
                hist_e[m].append(float(e0[m]))
            ri = cfg.record_interval
            for lo in range(0, cfg.n_sweeps, ri):
                hi = min(lo + ri, cfg.n_sweeps)
                eng.sweep(hi - lo, sched=temps[lo:hi])
                en = eng.energies().reshape(M, k).min(1)
                for m in range(M):
                    hist_e[m].append(float(en[m]))
            acc, att = eng.stats()
            out = []
            for m in range(M):
                cand = [eng.best(m * k + j) for j in range(k)]
                j = int(np.argmin([c[0] for c in cand]))
                rate = float(acc[m * k:(m + 1) * k].sum()) / float(max(att[m * k:(m + 1) * k].sum(), 1))
                out.append(AnnealingResult(
                    best_configuration=torch.from_numpy(cand[j][1].astype(np.float32)),
                    best_energy=cand[j][0], energy_history=hist_e[m],
                    temperature_history=[cfg.initial_temp] + [float(t) for t in temps[ri - 1::ri]],
                    acceptance_rate_history=[rate], total_time=(time.time() - t0) / M,
                    n_sweeps=cfg.n_sweeps, algorithm="simulated_annealing",
                    device=f"cuda:{self.device_index}", random_seed=cfg.random_seed))
        return out
