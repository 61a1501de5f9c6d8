"""The resampling step of population annealing (sga_resample, csrc/resample.hip) in plain Python integers: the rule is a
function of the energies, dbeta, the seed and a round number, with fixed-point weights and 128-bit compares, so Python's
own integers with the oracle's exp and Philox are an exact reference for it.  Shared by tests/test_resample_host.py and
tests/test_resample_gpu.py."""
from bisect import bisect_right

import numpy as np

import oracle

DOMAIN_RESAMPLE = 6  # DOMAIN_INIT | (1 << 2): the domain word of the step's one draw
MAX_MEMBERS = 1 << 23


def weights(E, dbeta):
    """(W list of ints, x_max) of one population: W_r = trunc(exp(x_r - x_max) * 2^40), x_r = (-dbeta) * E_r in fp64."""
    nb = -float(dbeta)
    x = [nb * float(e) for e in E]
    x_max = max(x)
    return [int(oracle.exp(v - x_max) * 2.0 ** 40) for v in x], x_max


def draw(seed, round_, gpop):
    """U = (word 0 << 32) | word 1 of Philox block (0, round, global population index, 6) under the engine's seed."""
    w = oracle.philox([0, int(round_) & 0xFFFFFFFF, int(gpop) & 0xFFFFFFFF, DOMAIN_RESAMPLE],
                      [int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF])
    return (int(w[0]) << 32) | int(w[1])


def counts_from(W, offset):
    """Children of every member under systematic resampling: child k sits at k S + offset, its parent is the r with
    N C_{r-1} <= t_k < N C_r."""
    N, S = len(W), sum(W)
    assert 0 <= offset < S
    NC, c = [], 0
    for w in W:
        c += w
        NC.append(N * c)
    n = [0] * N
    for k in range(N):
        n[bisect_right(NC, k * S + offset)] += 1
    return n


def place(counts):
    """parents[d] of the placement rule: a member with a child keeps its slot; the slots without one, ascending, take the
    surplus list (r repeated counts[r] - 1 times, ascending in r)."""
    N = len(counts)
    parents = list(range(N))
    surplus = [r for r in range(N) for _ in range(counts[r] - 1)]
    empty = [d for d in range(N) if counts[d] == 0]
    assert len(surplus) == len(empty)
    for d, r in zip(empty, surplus):
        parents[d] = r
    return parents


def plan(E, dbeta, seed, round_, gpop):
    """One population: (parents int32 [N] as indices into the population, shift = x_max, S, counts int64 [N])."""
    W, x_max = weights(E, dbeta)
    S = sum(W)
    assert len(W) <= MAX_MEMBERS and 2 ** 40 <= S < 2 ** 64
    offset = (draw(seed, round_, gpop) * S) >> 64
    n = counts_from(W, offset)
    return np.asarray(place(n), np.int32), float(x_max), S, np.asarray(n, np.int64)


def plan_all(E, dbeta, n_populations, seed, round_, replica0=0):
    """The whole call over R local replicas: (parents int32 [R] local indices, shift float64 [P], S uint64 [P])."""
    E = np.asarray(E, np.float64)
    P = int(n_populations)
    N = E.size // P
    db = np.broadcast_to(np.asarray(dbeta, np.float64), (P,))
    parents, shift, S = np.zeros(E.size, np.int32), np.zeros(P, np.float64), np.zeros(P, np.uint64)
    for p in range(P):
        par, shift[p], s, _ = plan(E[p * N:(p + 1) * N], db[p], seed, round_, replica0 // N + p)
        parents[p * N:(p + 1) * N] = par + p * N
        S[p] = s
    return parents, shift, S


def log_q(shift, S, N):
    """ln Q_p = shift[p] + ln(S_p / (N 2^40)) as the package forms it from the call's two exact outputs."""
    return np.asarray(shift, np.float64) + np.log(np.asarray(S, np.uint64).astype(np.float64) / (float(N) * 2.0 ** 40))


def apply(parents, spins, energy, best_energy=None, best_spins=None):
    """The state after the copy, in place: a destination takes its parent's spins and energy; its best follows where the
    parent's energy is below it."""
    src = np.asarray(parents)
    dst = np.nonzero(src != np.arange(src.size))[0]
    if best_energy is not None:
        for d in dst:
            if energy[src[d]] < best_energy[d]:
                best_energy[d] = energy[src[d]]
                best_spins[d] = spins[src[d]]
    spins[dst] = spins[src[dst]]
    energy[dst] = energy[src[dst]]


def run(prob, population_size, n_populations, betas, sweeps_per_step, seed, n_threads=1):
    """Population annealing on the CPU oracle, the loop of PopulationAnnealing.run: random spins at beta = 0; per step the
    plan of round `step`, the copy, sweeps_per_step sweeps at 1 / betas[step + 1] continuing the sweep counter.  Returns
    dict(parents [steps, R], energy [R], spins [R, n], log_partition [P], mean_energy [steps] of population 0)."""
    N, P = int(population_size), int(n_populations)
    R, n = N * P, prob.n
    betas = np.asarray(betas, np.float64)
    steps = betas.size - 1
    spins = oracle.init_spins(n, R, seed)
    energy = oracle.energy(prob, spins)
    log_z = np.full(P, n * np.log(2.0))
    hist, mean_e = np.zeros((steps, R), np.int32), []
    for step in range(steps):
        parents, shift, S = plan_all(energy, betas[step + 1] - betas[step], P, seed, step)
        apply(parents, spins, energy)
        out = oracle.sweeps(prob, spins, 1.0 / betas[step + 1], int(sweeps_per_step), seed=seed, energy=energy,
                            sweep0=step * int(sweeps_per_step), n_threads=n_threads)
        energy = out["energy"]
        log_z = log_z + log_q(shift, S, N)
        hist[step] = parents
        mean_e.append(float(energy[:N].mean()))
    return dict(parents=hist, energy=energy, spins=spins, log_partition=log_z, mean_energy=mean_e)
