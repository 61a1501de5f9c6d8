#!/usr/bin/env python3
"""The reference's annealing entry points on the MI355X engine: an import switch.

    # from spin_glass_rl.core.ising_model import IsingModel, IsingModelConfig
    # from spin_glass_rl.annealing.gpu_annealer import GPUAnnealer, GPUAnnealerConfig
    # from spin_glass_rl.annealing.parallel_tempering import ParallelTempering, ParallelTemperingConfig
    from spin_glass_anneal_rl_amd import ...

Needs an MI355X (there is no CPU fallback).  Run from the repository root:  python examples/hot_path_usage.py
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spin_glass_anneal_rl_amd import (GPUAnnealer, GPUAnnealerConfig, IsingModel, IsingModelConfig,  # noqa: E402
                                      ParallelTempering, ParallelTemperingConfig, PopulationAnnealing,
                                      PopulationAnnealingConfig, SpinGlassScheduler)
from spin_glass_anneal_rl_amd import encoders  # noqa: E402


def random_pm1_model(n, seed):
    g = torch.Generator().manual_seed(seed)
    J = (torch.randint(0, 2, (n, n), generator=g) * 2 - 1).float().triu(1)
    model = IsingModel(IsingModelConfig(n_spins=n, use_sparse=False, device="cuda"))
    model.set_couplings_from_matrix(J + J.T)
    return model


def simulated_annealing():
    model = random_pm1_model(256, seed=1)
    print(f"initial energy {model.compute_energy():.1f}")
    result = GPUAnnealer(GPUAnnealerConfig(n_sweeps=2000, random_seed=7)).anneal(model)
    print(f"SA: best energy {result.best_energy:.1f} after {result.n_sweeps} sweeps in {result.total_time:.3f} s")


def parallel_tempering():
    model = random_pm1_model(64, seed=1)
    cfg = ParallelTemperingConfig(n_replicas=8, n_sweeps=1000, exchange_interval=10, random_seed=42)
    result = ParallelTempering(cfg).run(model)
    print(f"PT: best energy {result.best_energy:.1f} in {result.total_time:.3f} s")


def many_replicas():
    model = random_pm1_model(2048, seed=3)
    t = time.time()
    result = SpinGlassScheduler(device="cuda", random_seed=5).anneal(model, n_replicas=1024, n_sweeps=300)
    dt = time.time() - t
    print(f"1024 replicas x 2048 spins x 300 sweeps: best energy {result.best_energy:.1f}, "
          f"{1024 * 2048 * 300 / dt:.3g} spin-flip attempts/s")


def many_models():
    """Independent models through one engine; with the field cache on, each replica keeps its local fields resident and
    reads a coupling row of ITS model on accept only (same results as field_cache="off")."""
    from spin_glass_anneal_rl_amd import BatchConfig, BatchProcessor
    models = [random_pm1_model(1024, seed=10 + i) for i in range(8)]
    cfg = GPUAnnealerConfig(n_sweeps=500, random_seed=3, field_cache="on")
    t = time.time()
    results = BatchProcessor(cfg, BatchConfig(replicas_per_model=2)).process_models_batch(models)
    print(f"batch of {len(models)} models, field cache on: best energies "
          f"{[round(r.best_energy) for r in results]} in {time.time() - t:.3f} s")


def one_graph_many_fields():
    """One coupling matrix under many field vectors -- bias vectors a policy proposes, clamped sub-problems, a field
    scan: BatchConfig(shared_couplings=True) hands the matrix over once (sga_set_dense_shared), each model contributes
    its h alone.  Same results as the default (stacked) path; the engine holds J once."""
    from spin_glass_anneal_rl_amd import BatchConfig, BatchProcessor
    base = random_pm1_model(1024, seed=20)
    g = torch.Generator().manual_seed(21)
    models = []
    for _ in range(8):
        m = IsingModel(IsingModelConfig(n_spins=1024, use_sparse=False, device="cuda"))
        m.set_couplings_from_matrix(base.dense_couplings())
        m.set_external_fields(torch.randint(-1, 2, (1024,), generator=g).float())
        models.append(m)
    cfg = GPUAnnealerConfig(n_sweeps=500, random_seed=3)
    bp = BatchProcessor(cfg, BatchConfig(replicas_per_model=2, shared_couplings=True))
    t = time.time()
    results = bp.process_models_batch(models)
    print(f"one graph, {len(models)} field vectors: best energies {[round(r.best_energy) for r in results]} in "
          f"{time.time() - t:.3f} s\n  engine: {bp.last_description}")


def one_sparse_graph_many_fields(L=12, n_fields=8, n_replicas=4):
    """A random-field scan over one 3-D +-J lattice: the CSR rows go to the engine once (AnnealEngine.set_csr_shared),
    each model is a field vector; every model walks the chain a one-model engine would walk."""
    from spin_glass_anneal_rl_amd import AnnealEngine
    rs = np.random.RandomState(2)
    idx = np.arange(L ** 3).reshape(L, L, L)
    J = np.zeros((L ** 3, L ** 3), np.float32)
    for ax in range(3):
        a, b = idx.ravel(), np.roll(idx, -1, axis=ax).ravel()
        J[a, b] = J[b, a] = rs.randint(0, 2, a.size) * 2.0 - 1.0
    rowptr = np.concatenate([[0], np.cumsum((J != 0).sum(1))]).astype(np.int32)
    colidx = np.concatenate([np.nonzero(r)[0] for r in J]).astype(np.int32)
    val = J[J != 0].astype(np.float32)
    H = np.stack([w * rs.choice([-1.0, 1.0], L ** 3) for w in range(n_fields)]).astype(np.float32)  # field strength 0, 1, 2, ...
    with AnnealEngine(0) as e:
        e.set_csr_shared(rowptr, colidx, val, H)
        e.init_replicas(n_fields * n_replicas, seed=5)
        e.set_ladder(np.tile(np.geomspace(3.0, 0.3, n_replicas), n_fields), n_ladders=n_fields)
        for _ in range(20):
            e.sweep(10)
            e.exchange(count=False)
        best = [min(e.best(m * n_replicas + j)[0] for j in range(n_replicas)) for m in range(n_fields)]
        print(f"one lattice, {n_fields} field strengths: best energies {[round(b) for b in best]}\n  engine: {e.describe()}")


def frustrated_lattice_with_cluster_moves(L=10):
    """Parallel tempering on a 3-D +-J lattice with isoenergetic cluster moves: two copies of the ladder run side by side,
    and after every exchange round the copies trade, slot by slot, the connected component of differing sites around
    one drawn site (AnnealEngine.cluster_move_ladders) -- rejection free, E_a + E_b conserved, sparse couplings only.
    measure_overlaps: after each of those rounds, from sweep 100 on, the spin and link overlap between the copies goes
    into histograms per temperature that stay on the device (AnnealEngine.accumulate_ladder_overlaps)."""
    rs = np.random.RandomState(4)
    idx = np.arange(L ** 3).reshape(L, L, L)
    J = np.zeros((L ** 3, L ** 3), np.float32)
    for ax in range(3):
        a, b = idx.ravel(), np.roll(idx, -1, axis=ax).ravel()
        J[a, b] = J[b, a] = rs.randint(0, 2, a.size) * 2.0 - 1.0
    model = IsingModel(IsingModelConfig(n_spins=L ** 3, use_sparse=True))
    model.set_couplings_from_matrix(torch.from_numpy(J))
    cfg = ParallelTemperingConfig(n_replicas=16, n_sweeps=500, temp_min=0.2, temp_max=3.0, exchange_interval=10, random_seed=42,
                                  n_copies=2, cluster_moves=True, cluster_temp_max=1.2,
                                  measure_overlaps=True, measure_after=100, overlap_bins=64)
    pt = ParallelTempering(cfg)
    result = pt.run(model)
    print(f"PT + cluster moves, {L}^3 +-J lattice: best energy {result.best_energy:.1f}; {pt.cluster_moves_flipped} of "
          f"{pt.cluster_moves_made} moves flipped {pt.cluster_sites_flipped} sites, largest cluster {pt.cluster_size_max}")
    st = pt.overlap_statistics
    print(f"  overlaps between the copies over {pt.overlap_rounds_measured} rounds, coldest / hottest temperature: <q^2> "
          f"{st.moments()[0][-1]:.3f} / {st.moments()[0][0]:.3f}, Binder {st.binder()[-1]:.2f} / {st.binder()[0]:.2f}, "
          f"link overlap {st.link_overlap()[-1]:.3f} / {st.link_overlap()[0]:.3f}")


def frustrated_lattice_correlation_length(L=8):
    """The finite-size correlation length xi_L / L of a 3-D +-J lattice per temperature, the quantity whose crossing locates
    T_c: two copies of the ladder, and after every exchange round from sweep 200 on the overlap between the copies resolved
    by the lattice's planes goes, with its second moments, into sums that stay on the device
    (AnnealEngine.accumulate_ladder_class_overlaps with the class maps of encoders.lattice_planes)."""
    rs = np.random.RandomState(4)
    idx = np.arange(L ** 3).reshape(L, L, L)
    J = np.zeros((L ** 3, L ** 3), np.float32)
    for ax in range(3):
        a, b = idx.ravel(), np.roll(idx, -1, axis=ax).ravel()
        J[a, b] = J[b, a] = rs.randint(0, 2, a.size) * 2.0 - 1.0
    model = IsingModel(IsingModelConfig(n_spins=L ** 3, use_sparse=True))
    model.set_couplings_from_matrix(torch.from_numpy(J))
    cfg = ParallelTemperingConfig(n_replicas=12, n_sweeps=1000, temp_min=0.6, temp_max=2.4, exchange_interval=10, random_seed=42,
                                  n_copies=2, measure_class_overlaps=True, overlap_classes=encoders.lattice_planes((L, L, L)),
                                  measure_after=200)
    pt = ParallelTempering(cfg)
    pt.run(model)
    st = pt.class_overlap_statistics
    print(f"PT, {L}^3 +-J lattice, plane overlaps over {st.measurements} rounds: xi_L / L per temperature")
    for T, xi in zip(st.temperatures, st.correlation_length() / L):
        print(f"  T = {T:.3f}  xi_L / L = {xi:.3f}")


def frustrated_lattice_by_population_annealing(L=8):
    """Population annealing on a 3-D +-J lattice: 4 independent populations of 1024 replicas cooled together from beta = 0
    to 2, every replica copied or culled by its weight at each step (AnnealEngine.resample, on the device).  The run yields
    the free energy -- the spread over the populations is its error bar -- and the surviving families say whether the
    population equilibrated."""
    rs = np.random.RandomState(4)
    idx = np.arange(L ** 3).reshape(L, L, L)
    J = np.zeros((L ** 3, L ** 3), np.float32)
    for ax in range(3):
        a, b = idx.ravel(), np.roll(idx, -1, axis=ax).ravel()
        J[a, b] = J[b, a] = rs.randint(0, 2, a.size) * 2.0 - 1.0
    model = IsingModel(IsingModelConfig(n_spins=L ** 3, use_sparse=True))
    model.set_couplings_from_matrix(torch.from_numpy(J))
    pa = PopulationAnnealing(PopulationAnnealingConfig(population_size=1024, n_populations=4, beta_max=2.0, n_steps=40,
                                                       sweeps_per_step=5, random_seed=42))
    result = pa.run(model)
    f, err = pa.free_energy.mean() / L ** 3, pa.free_energy.std(ddof=1) / 2.0 / L ** 3
    print(f"population annealing, {L}^3 +-J lattice: best energy {result.best_energy:.1f}; free energy per spin at beta = 2: "
          f"{f:.4f} +- {err:.4f}; families left {pa.family_counts.tolist()} of 1024, rho_t {np.round(pa.rho_t, 1).tolist()}")


def frustrated_lattice_by_simulated_quantum_annealing(L=8):
    """Simulated quantum annealing on a 3-D +-J lattice, the upstream README's call: 32 Trotter slices of the instance are
    32 replicas coupled along imaginary time inside the sweep (AnnealEngine.sweep_transverse, on the device), the transverse
    field falls from 3 to 0.01, and the best is the lowest CLASSICAL energy any slice met."""
    from spin_glass_anneal_rl_amd.quantum import QuantumFluctuations
    rs = np.random.RandomState(4)
    idx = np.arange(L ** 3).reshape(L, L, L)
    J = np.zeros((L ** 3, L ** 3), np.float32)
    for ax in range(3):
        a, b = idx.ravel(), np.roll(idx, -1, axis=ax).ravel()
        J[a, b] = J[b, a] = rs.randint(0, 2, a.size) * 2.0 - 1.0
    model = IsingModel(IsingModelConfig(n_spins=L ** 3, use_sparse=True))
    model.set_couplings_from_matrix(torch.from_numpy(J))
    annealer = GPUAnnealer(GPUAnnealerConfig(n_sweeps=2000, final_temp=0.05, random_seed=42, record_interval=100))
    quantum_annealer = QuantumFluctuations(base_annealer=annealer, transverse_field_schedule="linear_decrease",
                                           initial_field_strength=3.0)
    sqa = quantum_annealer.simulated_quantum_anneal(model, n_trotter_slices=32, quantum_monte_carlo=True)
    pimc = quantum_annealer.path_integral_mc(model, imaginary_time_slices=64, quantum_temperature=0.1)
    # towards Gamma = 0.01 the slices freeze into copies; world-line cluster updates (AnnealEngine.worldline_clusters) after
    # every transverse sweep keep them moving
    with_clusters = QuantumFluctuations(base_annealer=annealer, transverse_field_schedule="linear_decrease",
                                        initial_field_strength=3.0, worldline_clusters=True)
    sqa_clusters = with_clusters.simulated_quantum_anneal(model, n_trotter_slices=32)
    print(f"SQA, {L}^3 +-J lattice, 32 slices: best energy {sqa.best_energy:.1f} in {sqa.total_time:.3f} s; "
          f"PIMC at Gamma = 3, 64 slices: best energy {pimc.best_energy:.1f}")
    # equilibrium path-integral Monte Carlo on a ladder of transverse fields: 8 instances at 0.93 ... 1.07 Gamma, an exchange
    # between neighbouring instances after every 5th sweep (AnnealEngine.exchange_transverse, decided on the device on the
    # broken time links of AnnealEngine.time_links); <sigma^x> of every instance comes from the same counts
    ladder = QuantumFluctuations(base_annealer=annealer, transverse_field_schedule="constant", initial_field_strength=1.0,
                                 n_instances=8, field_ladder=np.geomspace(0.93, 1.07, 8).tolist(), field_exchange_interval=5)
    pt = ladder.path_integral_mc(model, imaginary_time_slices=32, quantum_temperature=0.05)
    attempts, accepts = ladder.last.field_exchange_statistics
    print(f"   PIMC on a ladder of 8 fields: best energy {pt.best_energy:.1f}; exchanges accepted per pair "
          f"{np.round(accepts / np.maximum(attempts, 1), 2).tolist()}; <sigma^x> {np.round(ladder.last.transverse_magnetization, 3).tolist()}")


def sk_glass_by_simulated_quantum_annealing(n=1024):
    """The same call on a fully connected +-1 (SK-type) instance: dense_couplings=True hands the matrix over dense with the
    field cache on and sweeps through AnnealEngine.sweep_transverse_dense -- a slice's local fields resident in LDS, a
    coupling row read only when a proposal is accepted.  Without the flag a dense model is refused (no classical fallback)."""
    from spin_glass_anneal_rl_amd.quantum import QuantumFluctuations
    model = random_pm1_model(n, seed=5)
    annealer = GPUAnnealer(GPUAnnealerConfig(n_sweeps=500, final_temp=0.05, random_seed=42, record_interval=50))
    quantum_annealer = QuantumFluctuations(base_annealer=annealer, transverse_field_schedule="linear_decrease",
                                           initial_field_strength=3.0 * np.sqrt(n), final_field_strength=0.05,
                                           n_instances=4, dense_couplings=True)
    sqa = quantum_annealer.simulated_quantum_anneal(model, n_trotter_slices=32, quantum_monte_carlo=True)
    print(f"SQA, dense +-1 couplings on {n} spins, 4 instances x 32 slices: best energy {sqa.best_energy:.1f} "
          f"({sqa.best_energy / n ** 1.5:.4f} n^1.5) in {sqa.total_time:.3f} s")
    # the cluster move beside the dense sweep (AnnealEngine.worldline_clusters_dense): decided on the same cached fields,
    # which stay valid between the two calls -- a coupling row is read only where a segment of slices flips
    with_clusters = QuantumFluctuations(base_annealer=annealer, transverse_field_schedule="linear_decrease",
                                        initial_field_strength=3.0 * np.sqrt(n), final_field_strength=0.05,
                                        n_instances=4, dense_couplings=True, dense_worldline_clusters=True)
    sqa_c = with_clusters.simulated_quantum_anneal(model, n_trotter_slices=32)
    print(f"   with world-line clusters after every sweep: best energy {sqa_c.best_energy:.1f} in {sqa_c.total_time:.3f} s; "
          f"segments formed / flipped, slice spins flipped: {with_clusters.last.cluster_statistics.tolist()}")


def travelling_salesman(n_cities=12):
    rs = np.random.RandomState(0)
    xy = rs.rand(n_cities, 2)
    d = np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1])
    builder = encoders.tsp_ising(d, city_visit=4.0, position_fill=4.0)
    model = builder.to_model(sparse=False)
    result = SpinGlassScheduler(device="cuda", random_seed=1).anneal(
        model, n_replicas=256, n_sweeps=2000, beta_min=0.5, beta_max=50.0)
    x = (result.best_configuration.numpy().reshape(n_cities, n_cities) > 0)
    feasible = (x.sum(0) == 1).all() and (x.sum(1) == 1).all()
    length = result.best_energy + builder.penalty_energy_offset()
    print(f"TSP, {n_cities} cities: objective + penalties = {length:.3f}, one-hot constraints satisfied: {bool(feasible)}")
    if feasible:
        tour = [int(np.argmax(x[:, p])) for p in range(n_cities)]
        print("   tour:", tour)


def scheduling_without_storing_couplings(n_tasks=500, n_slots=100, n_replicas=1024, n_sweeps=100):
    """A scheduling instance whose every coupling comes from a cardinality constraint (one start per task, one task
    per slot): the engine keeps the groups and their sums instead of J (AnnealEngine.set_groups), bit-identical to
    the stored-coupling chain -- 0.8 MB of tables instead of 256 MB of CSR at this size."""
    from spin_glass_anneal_rl_amd import AnnealEngine
    from spin_glass_anneal_rl_amd.encoders import scheduling_groups
    n, member_ptr, members, coeff, h, constant = scheduling_groups(
        np.full(n_tasks, 1.0), 1, float(n_slots), n_slots, objective="total_time",
        penalty_weights={"assignment": 100.0, "capacity": 50.0})
    with AnnealEngine(0) as eng:
        eng.set_groups(n, (member_ptr, members), coeff, h)
        eng.init_replicas(n_replicas, seed=3)
        eng.set_ladder(np.geomspace(500.0, 5.0, n_replicas), 1)
        for _ in range(n_sweeps // 10):
            eng.sweep(10)
            eng.exchange(count=False)
        energy, spins, replica = eng.best()
        return energy + constant, spins, eng.describe()


def scheduling_with_precedence_as_groups_plus_remainder(n_tasks=500, n_slots=100, n_replicas=1024, n_sweeps=100):
    """The same instance with precedence terms along a chain of tasks: the cardinality constraints stay groups, the
    precedence couplings are handed over as a stored sparse remainder (AnnealEngine.set_groups(..., rest=)) -- the
    constraints still cost no coupling bytes, bit-identical to the stored-coupling chain."""
    from spin_glass_anneal_rl_amd import AnnealEngine
    from spin_glass_anneal_rl_amd.encoders import scheduling_groups_rest
    n, member_ptr, members, coeff, rest, h, constant = scheduling_groups_rest(
        np.full(n_tasks, 1.0), 1, float(n_slots), n_slots, {"assignment": 100.0, "capacity": 50.0, "precedence": 80.0},
        objective="total_time", precedence_pairs=[(t, t + 1) for t in range(n_tasks - 1)])
    with AnnealEngine(0) as eng:
        eng.set_groups(n, (member_ptr, members), coeff, h, rest=rest)
        eng.init_replicas(n_replicas, seed=3)
        eng.set_ladder(np.geomspace(500.0, 5.0, n_replicas), 1)
        for _ in range(n_sweeps // 10):
            eng.sweep(10)
            eng.exchange(count=False)
        energy, spins, replica = eng.best()
        return energy + constant, spins, eng.describe()


def travelling_salesman_without_storing_couplings(n_cities=200, n_replicas=512, n_sweeps=200):
    """The same QUBO at a size where the couplings themselves become the cost (200 cities: 40 000
    spins, 32 M couplings; 1000 cities: 10^6 spins, 32 GB): the engine keeps distances + penalty
    weights and rebuilds a row's sum from the TSP structure (AnnealEngine.set_tsp), bit-identical
    to the stored-coupling chain."""
    from spin_glass_anneal_rl_amd import AnnealEngine
    rs = np.random.RandomState(1)
    xy = rs.rand(n_cities, 2) * 100.0
    d = np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1])
    dist, w_city, w_pos, h, constant = encoders.tsp_structure(d, city_visit=200.0, position_fill=200.0)
    n_ladders = 8
    ladder = np.tile(np.geomspace(200.0, 2.0, n_replicas // n_ladders), n_ladders)
    with AnnealEngine(0) as eng:
        eng.set_tsp(dist, w_city, w_pos, h)
        eng.init_replicas(n_replicas, seed=3)
        eng.set_ladder(ladder, n_ladders)
        t = time.time()
        for _ in range(n_sweeps // 10):
            eng.sweep(10)
            eng.exchange(count=False)
        best, spins, _ = eng.best()
        dt = time.time() - t
    print(f"TSP, {n_cities} cities without stored couplings: best objective + penalties = {best + constant:.1f}, "
          f"{n_replicas * n_cities ** 2 * n_sweeps / dt:.3g} spin-flip attempts/s ({eng_desc(n_cities)})")


def eng_desc(n_cities):
    return f"{n_cities ** 2} spins, {4 * (n_cities - 1) * n_cities ** 2 / 1e6:.0f} M couplings never materialised"


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("this example needs an MI355X")
    simulated_annealing()
    parallel_tempering()
    many_replicas()
    many_models()
    one_graph_many_fields()
    one_sparse_graph_many_fields()
    frustrated_lattice_with_cluster_moves()
    frustrated_lattice_correlation_length()
    frustrated_lattice_by_population_annealing()
    frustrated_lattice_by_simulated_quantum_annealing()
    sk_glass_by_simulated_quantum_annealing()
    travelling_salesman()
    travelling_salesman_without_storing_couplings()
    scheduling_without_storing_couplings()
    scheduling_with_precedence_as_groups_plus_remainder()
