/*
 * sga.h -- C ABI of the MI355X (gfx950) digital-annealing engine: the drop-in boundary for
 * the reference's Ising spin-sweep hot path.  Plain C, opaque handle, int status returns,
 * no torch types.  Shared library: spin-glass-anneal-rl_amd/csrc/libsga.so.
 *
 * What each entry point replaces in the reference (paths relative to the reference root):
 *
 *   sga_set_dense / sga_set_csr   IsingModel.couplings / external_fields buffers handed to the
 *                                 kernels: spin_glass_rl/annealing/cuda_kernels.py:228-236
 *                                 (dense fp32 [n,n]); core/ising_model.py:69-84 (dense | COO)
 *   sga_init_replicas             ParallelTempering._initialize_replicas,
 *                                 annealing/parallel_tempering.py:175-189 (copy + reset_to_random)
 *   sga_sweep                     CUDAKernelManager.metropolis_update_optimized,
 *                                 annealing/cuda_kernels.py:228-282 (+ fallback :371-398) and
 *                                 SpinDynamics.sweep, core/spin_dynamics.py:73-94, batched over
 *                                 replicas (ParallelTempering._parallel_sweeps, :191-203)
 *   sga_recompute_energies        CUDAKernelManager.compute_energy_optimized,
 *                                 annealing/cuda_kernels.py:284-324 (+ fallback :400-413);
 *                                 IsingModel.compute_energy, core/ising_model.py:149-174
 *   sga_exchange                  CUDAKernelManager.parallel_tempering_exchange_optimized,
 *                                 annealing/cuda_kernels.py:326-369 (+ fallback :415-443) and
 *                                 ParallelTempering._nearest_neighbor_exchange /
 *                                 _attempt_single_exchange, annealing/parallel_tempering.py:214-258
 *   sga_local_fields              IsingModel.get_local_field, core/ising_model.py:176-185
 *   sga_flip                      IsingModel.flip_spin, core/ising_model.py:125-147
 *   sga_update                    SpinDynamics.single_spin_update / _metropolis_update,
 *                                 core/spin_dynamics.py:61-71,131-152
 *   sga_get_best                  best tracking in GPUAnnealer.anneal, gpu_annealer.py:151-153,
 *                                 and ParallelTempering._find_best_solution, :303-313
 *   sga_get_stats                 SpinDynamics.n_accepted / n_rejected, spin_dynamics.py:44-45
 *
 * Pointers: every user buffer may be a host pointer or a device pointer on the engine's device
 * (copies use hipMemcpyDefault); PyTorch-ROCm tensors are passed as tensor.data_ptr().  J / h
 * are packed into engine-owned HBM at set time (device buffers are read in place, never copied
 * whole), so the caller's tensors are not borrowed after the call returns.  Calls on one handle must be serialised by the caller; different
 * handles are independent.  No call throws; on failure a negative code is returned and
 * sga_last_error() (thread-local) describes it.
 */
#ifndef SGA_H
#define SGA_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sga_engine sga_engine;

/* status codes */
#define SGA_OK 0
#define SGA_ERR_INVALID -1 /* bad argument / state  -> AnnealingError in the Python shim   */
#define SGA_ERR_DEVICE -2  /* no / invalid GPU, HIP failure -> DeviceError                 */
#define SGA_ERR_MEMORY -3  /* allocation failure                                           */
#define SGA_ERR_UNSUPPORTED -4

/* coupling storage in HBM */
#define SGA_J_AUTO 0 /* bit-planes if J is ternary and n >= 4096, int8 if integer in [-127,127], else fp32;
                        * a sparse integer matrix (n >= 4096, <= 256 non-zeros per row) is kept as CSR when the
                        * field cache is OFF, or AUTO on a problem the cached-field sweep cannot serve */
#define SGA_J_F32 1
#define SGA_J_I8 2
#define SGA_J_T2 3 /* J in {-1,0,+1} as two bit-planes (sign, non-zero): 2 bits per coupling */

/* site order of a sweep */
#define SGA_SITE_RANDOM 0     /* uniform with replacement, Philox4x32-10 (spin_dynamics.py:69) */
#define SGA_SITE_SEQUENTIAL 1 /* i = 0..n-1 (cuda_kernels.py:381)                             */
#define SGA_SITE_REPLAY 2     /* caller-supplied sites (parity tests)                         */

/* arithmetic of the accept rule */
#define SGA_ARITH_F64 0 /* spin_dynamics.py:131-152 (double dE, fp32 exp)                     */
#define SGA_ARITH_F32 1 /* cuda_kernels.py:383-390 (fp32 throughout, minus J_ii s_i)          */

/* single-site update rule (core/spin_dynamics.py:11-16) used by sga_sweep / sga_update */
#define SGA_RULE_METROPOLIS 0 /* spin_dynamics.py:131-152                                      */
#define SGA_RULE_GLAUBER 1    /* spin_dynamics.py:154-171: s_i = +1 w.p. 1/(1+exp(-2 f/T))     */
#define SGA_RULE_HEAT_BATH 2  /* spin_dynamics.py:173-191: same with beta = 1/T formed first   */
#define SGA_RULE_WOLFF 3      /* spin_dynamics.py:193-255: cluster moves (sga_sweep only)         */

/* ---- lifetime ------------------------------------------------------------------------- */
int sga_create(int device, sga_engine **out);
void sga_destroy(sga_engine *e);
const char *sga_last_error(void);
int sga_version(void);  /* 3400: sga_sweep_transverse_dense serves real-valued dense couplings too, on the fixed-point cached fields of option "clf_fixed_point" (D = 2^k J s as exact int32 | int64, any fp32 h; csrc/sweep_transverse_fx.hip; no new entry point, no new option); 3300: sga_get_time_links / sga_exchange_transverse (simulated quantum annealing: the broken time links of every Trotter group counted on the device, and one round of replica exchange between neighbouring groups along the transverse field decided on those counts, csrc/trotter_exchange.hip; domain word 8; no option, no engine member); 3200: sga_worldline_clusters_dense (world-line cluster updates on dense couplings: the step of sga_worldline_clusters decided on the resident fields of every slice, a coupling row read only where a segment flips, the fields kept valid, csrc/worldline_clusters_dense.hip; no option, no engine member); 3100: sga_sweep_transverse_dense (simulated quantum annealing on dense couplings: the step of sga_sweep_transverse carried by the cached local fields, a coupling row read on accept only, csrc/sweep_transverse_clf.hip; no option, no engine member); 3000: sga_worldline_clusters (simulated quantum annealing: Swendsen-Wang clusters along imaginary time at one site, flipped under the classical field, one launch per call, csrc/worldline_clusters.hip; domain word 4; no option, no engine member); 2900: sga_sweep_transverse (simulated quantum annealing: the Trotter slices of one instance coupled in the CSR sweep, two half-sweeps per sweep, csrc/sweep_transverse.hip; no option, no engine member); 2800: sga_get_class_overlaps / sga_accumulate_ladder_class_overlaps (the overlap between two replicas resolved by a class of sites, first and second moments per temperature summed on the device, csrc/class_overlaps.hip; read only, no engine state, no option); 2700: sga_get_link_count / sga_get_pair_overlaps / sga_accumulate_ladder_overlaps (spin and link overlaps between pairs of replicas, histogrammed per temperature on the device, csrc/pair_overlaps.hip; read only, no engine state, no option); 2600: sga_resample (the resampling step of population annealing, csrc/resample.hip); 2500: sga_cluster_move_pairs / sga_cluster_move_ladders (isoenergetic cluster moves between replica copies on sparse couplings, csrc/cluster_moves.hip; no engine state, no option); 2400: sga_set_replica_groups / sga_get_replica_groups; 2300: sga_get_magnetizations / sga_get_overlaps / sga_get_overlaps_with (replica observables on the device: the exact integer product of int8 spin rows on the matrix cores, csrc/observables.hip; read only, no engine state); 2200: the row-shared fields in tiles take a plan of their own, one launch per sweep (csrc/sweep_dense_rs.hip, rs_tile_plan_kernel; no change of interface or results); 2100: sga_set_sequential_windows / sga_get_sequential_windows (SGA_SITE_SEQUENTIAL sweeps in windows, the fields of every replica on the matrix cores; csrc/sweep_dense_seq.hip); 2000: the row-shared windows (option "row_shared") serve SGA_RULE_GLAUBER and SGA_RULE_HEAT_BATH too ("rule=glauber" / "rule=heat-bath" in sga_describe and sga_get_last_kernel; the window sga_autotune picks holds for the rule it was timed under); 1900: options "row_shared_fields" and "row_shared_tile_sites" (row-shared fields in tiles of sites, sign-only rows); 1800: option "row_shared_grid", sga_route_query.rs_grid; 1700: sga_set_csr_shared (one set of CSR rows, many field vectors: every one-wave-per-replica CSR form for such batches), sga_route_query.shared_j on SGA_ROUTE_CSR queries; 1600: sga_set_dense_shared (one coupling matrix, many field vectors; row-shared windows, bit-planes and the matrix-core pass for such batches), sga_route_query.shared_j; 1500: sga_get_scan_summary, and sga_set_dense / sga_set_dense_batch / sga_set_csr / sga_set_csr64 / sga_set_csr_batch refuse a NaN or +-Inf in J or h (SGA_ERR_INVALID, "non-finite"); 1400: option "batch_fixed_point" (fixed-point cached local fields for many-model dense batches); 1300: options "ragged_field_cache" and "clf_fixed_point" together (fixed-point cached local fields for ragged CSR batches); 1200: sga_set_groups_csr (group couplings plus a stored sparse remainder); 1100: option "ragged_field_cache" (cached local fields for ragged CSR batches); 1000: sga_set_groups */
/* Run on an existing HIP stream (e.g. torch.cuda.current_stream().cuda_stream); NULL = the
 * engine's own stream (default). */
int sga_set_stream(sga_engine *e, void *hip_stream);

/* ---- problem -------------------------------------------------------------------------- */
/* Dense couplings J[n][ldJ] (fp32, row-major, symmetric as the reference stores them) and
 * fields h[n]. */
int sga_set_dense(sga_engine *e, const float *J, int64_t ldJ, const float *h, int n,
                  int storage);
/* A batch of n_models independent dense problems of the same size (the reference's
 * BatchProcessor workload, annealing/batch_processor.py:231-288): J is the models' matrices
 * stacked row-wise, [n_models*n][ldJ]; h is [n_models][n].  Replicas are split evenly over
 * the models (global replica g belongs to model g / (R_global / n_models)); with a ladder,
 * use n_ladders = n_models so that exchanges stay inside a model.
 * sga_set_field_cache(ON / AUTO) serves a batch (version >= 900) whose stacked rows qualify as a whole: every
 * model's J integer valued and symmetric with a zero diagonal, every h in multiples of 1/2, the largest
 * sum_j |J_ij| + |h_i| of ANY model below 2^24.  Scale, field width (int16 | int32), accept table and max |J| are
 * batch-wide; each replica reads its own model's rows, and each model walks its one-model chain.  The fixed-point
 * form (option "clf_fixed_point"), bit-plane storage and row-shared windows stay one-model only -- the fixed-point form
 * unless option "batch_fixed_point" = 1 is set too (version >= 1400, both set before this call): a batch the integer
 * form does not take (real-valued J, an h off the half-integers) is then scanned as a whole for the fixed-point form.
 * k is batch-wide -- the finest grid 2^-k any model's J needs (0 for integer J), so every 2^k J of every model is an
 * integer --, the fields D = 2^k J_m s are int32 while 2^k max (sum_j |J_ij| + |h_i|) over ALL stacked rows < 2^31, else
 * int64.  dot = fp32(2^-k D_i) is the one rounding of the exact row sum: every model walks its one-model chain,
 * whatever k or width it would get alone.  Refused (SGA_ERR_UNSUPPORTED under SGA_FIELD_CACHE_ON, each naming "a dense
 * batch: in every model"): f64-canonical J over the stack, an asymmetric J or a non-zero diagonal in any model, fields
 * wider than int64.  A batch the integer form takes keeps it. */
int sga_set_dense_batch(sga_engine *e, const float *J, int64_t ldJ, const float *h, int n,
                        int n_models, int storage);
/* A batch with ONE coupling matrix and n_models field vectors (version >= 1600): J[n][ldJ] as in sga_set_dense, H is
 * [n_models][n] (the same graph under many bias vectors, clamped sub-problems, a field scan).  In every call of this
 * header the engine behaves exactly as after sga_set_dense_batch on J tiled n_models times with the same H -- the
 * replica -> model map g / (R_global / n_models), R_global % n_models != 0 refused, n_ladders = n_models,
 * sga_exchange_pairs (a pair across models is taken as there), spins, energies, bests, stats, export / import, the single-site operators,
 * sharding through replica0, every refusal and its wording, the eight words of sga_get_scan_summary -- and each model
 * walks the chain of a one-model engine holding (J, h_m) started at replica0 = m * (R_global / n_models), bit for bit,
 * in whatever form runs.  Four things differ:
 *   1. J is packed once: coupling memory is sga_set_dense's (bit-planes of the row-shared form included), not
 *      n_models times it.
 *   2. sga_problem_checksum covers J once and all of H.
 *   3. sga_describe / sga_explain_route name the kind: "shared-J models=M".
 *   4. The forms that need the ROWS to be the same for every replica open up: bit-plane storage (SGA_J_AUTO resolves
 *      as for one model -- bit-planes for ternary J from n = 4096, else int8, else fp32 -- and SGA_J_T2 is served),
 *      row-shared windows (option "row_shared"; integer J and EVERY h with exact fp32 sums -- one accept table for
 *      the batch --, symmetric J with a zero diagonal, |J| <= 255, production arguments, field cache OFF: a proposed
 *      row is read once for every replica of every model that proposes it; Metropolis decides with the accept table,
 *      Glauber and heat bath with the row kernels' general rule, Wolff is never served) and the matrix-core
 *      energy / field pass (J leaves HBM once for all replicas).  Cached fields ON / AUTO behave as on the stacked
 *      batch: batch-wide scale, field width and table; the fixed-point form behind "clf_fixed_point" +
 *      "batch_fixed_point".  AUTO's break-evens are the stacked batch's (not measured for shared batches).
 * A NaN or +-Inf in J or H: SGA_ERR_INVALID ("non-finite"), as the other setters. */
int sga_set_dense_shared(sga_engine *e, const float *J, int64_t ldJ, const float *H /* [n_models][n] */, int n,
                         int n_models, int storage);
/* CSR couplings (both triangles present), rowptr[n+1], colidx[nnz], val[nnz], h[n]; host or
 * device pointers.  The structure is checked on the device (SGA_ERR_INVALID for extents that are
 * not monotone / do not span [0, nnz], or a column outside [0, n)); rows need not be sorted and
 * duplicates add up.  The arrays are read where they lie (device) or through a staging copy (host)
 * and packed into the engine's layout -- (column, value) entries interleaved, rows of long-row
 * problems padded to whole 64-entry slots; the caller's buffers are not referenced after the call.
 * The same pass classifies how a row sum can be formed exactly (integer / fp64-exact / canonical
 * order, see sga_describe's "path=" and DESIGN.md 2).  Problems whose longest row has <= 64 entries
 * (lattices, low-degree graphs, BASELINE configs[2]) are swept several updates per step -- one per
 * row of 8 or 16 lanes, replayed one at a time when an accepted update touches a later one of the
 * step: the same chain, 3-6 x the one-update rate (sga_describe: "updates_per_step="). */
int sga_set_csr(sga_engine *e, const int32_t *rowptr, const int32_t *colidx, const float *val,
                const float *h, int n, int64_t nnz);
/* Same with 64-bit row extents, for nnz >= 2^31 (BASELINE config 5 at 1000 cities: n = 10^6,
 * nnz ~ 4e9; the reference's COO `couplings` tensor of core/ising_model.py:69-76 has no such
 * limit).  Problems whose int8 spins do not fit LDS (n > ~160k) keep them as bits, up to
 * n ~ 1.3e6; both cases are picked up automatically by sga_init_replicas. */
int sga_set_csr64(sga_engine *e, const int64_t *rowptr, const int32_t *colidx, const float *val,
                  const float *h, int n, int64_t nnz);

/* M independent CSR problems of any sizes in one engine (version >= 600).  n_spins[M] (host); rowptr[sum n + 1] is
 * ONE concatenated CSR: model m owns rows [row0_m, row0_m + n_m) with row0_m = n_0 + ... + n_{m-1}.  Its columns are
 * model-local (in [0, n_m)), and its fields are h[row0_m ...].  Host or device pointers, as sga_set_csr.  Replicas are
 * split evenly, as in sga_set_dense_batch: global replica g belongs to model g / (R_global / M) (R_global % M != 0 is
 * SGA_ERR_INVALID at sga_init_replicas); with a ladder, pass n_ladders = M (a multiple of M).
 *   Checks: sga_set_csr's per model (monotone extents, columns in [0, n_m), duplicates add up, unsorted rows allowed):
 *   SGA_ERR_INVALID naming the model.  A non-zero diagonal or an asymmetric J: SGA_ERR_UNSUPPORTED.  Layouts that
 *   need 64-bit extents, or a largest model beyond the narrow int8 form (~160 000 spins): SGA_ERR_UNSUPPORTED.
 *   Spins are [R][sstride(n_max)], zero past n_m: sga_get_spins(r >= 0) / sga_get_best / sga_set_spins move
 *   n_{model(r)} values, sga_get_spins(r < 0) writes [R_local][n_max] zero-padded, sga_init_replicas' s0 is
 *   [R_local][n_max] (padding ignored); s0 == NULL draws replica g as a one-model engine of n_{model(g)} spins would.
 *   Replay arrays and traces are [R][n_sweeps][n_max]: replica r uses the first n_{model(r)} entries of each sweep.
 *   Everything sga_sweep does (rules, site modes, traces, schedules), sga_exchange (n_ladders = M),
 *   sga_exchange_pairs (a pair across two models: SGA_ERR_INVALID), energies, sga_local_fields, best tracking,
 *   stats, export / import, the checksum (n_spins[] included), sga_describe ("csr batch models=M n=min..max ...") and
 *   the route calls work.  SGA_ERR_UNSUPPORTED: sga_set_field_cache(ON) (AUTO streams) unless option
 *   "ragged_field_cache" is set, the Wolff rule, sga_flip, sga_update, sga_autotune, and any option that would pick a
 *   wide, bit-spin or several-updates-per-step form.  One launch per sweep call: the narrow one-update form, each
 *   wave running its own model.
 *   Option "ragged_field_cache" = 1 (version >= 1100, set before this call): the batch is also scanned for the int16
 *   cached-field form of sga_set_csr -- in EVERY model J integer valued in strictly sorted rows without duplicates,
 *   h in multiples of 1/2, max_i sum_j |J_ij| < 2^15, rows of <= 2048 entries, the largest model within LDS -- and
 *   sga_set_field_cache(ON / AUTO) then acts as on a one-model CSR engine: one workgroup of 4 | 8 waves per replica,
 *   its model's fields D = J s resident in LDS, a row read on accept only.  Accept table, its scale and the launch
 *   geometry are batch-wide (the largest table, scale 2 as soon as one model has a half-integer h), which leaves
 *   every model on its one-model chain.  ON over a batch that does not qualify: sga_sweep fails with
 *   SGA_ERR_UNSUPPORTED naming the first offending model; AUTO streams there.
 *   Options "ragged_field_cache" = 1 and "clf_fixed_point" = 1 together (version >= 1300, both set before this call): a
 *   batch the int16 form does not take -- a model with real-valued J, an h that is no multiple of 1/2, integer fields
 *   of 2^15 or more -- is scanned for the fixed-point form of sga_set_csr: in EVERY model acc class f32 / f64-exact,
 *   strictly sorted rows without duplicates, rows of <= 2048 entries; any fp32 h (never folded into the fields).  k is
 *   batch-wide: the finest grid 2^-k any model's J needs, so every 2^k J of every model is an integer; the fields
 *   D = 2^k J_m s are int32 while 2^k max_i sum_j |J_ij| < 2^31 over all rows of the batch, else int64, and the batch
 *   is refused from 2^53 on.  dot = fp32(2^-k D_i) is one rounding of the exact row sum: every model walks its
 *   one-model chain.  A batch the int16 form takes keeps it.  Served by the cached kernel: SGA_SITE_RANDOM, both
 *   arithmetics, Metropolis / Glauber / heat bath, no per-update records; other calls take the streaming kernel and
 *   the fields are seeded anew.  sga_describe names "models=M", the width and k; refusals name the first offending
 *   model (f64-canonical J, unsorted or duplicate rows, a row too long, fields wider than the bound). */
int sga_set_csr_batch(sga_engine *e, int n_models, const int32_t *n_spins, const int64_t *rowptr,
                      const int32_t *colidx, const float *val, const float *h, int64_t nnz);
/* ONE set of CSR rows under n_models field vectors (version >= 1700): rowptr / colidx / val as in sga_set_csr, H is
 * [n_models][n] -- a random-field scan over one lattice, clamped sub-problems folded into h, one MaxCut or scheduling
 * instance under many penalty or bias settings.  sga_set_csr_batch on the rows written n_models times stores the
 * entries n_models times and runs the narrow one-update int8 form only; here the rows are checked, classified and
 * packed ONCE, exactly as sga_set_csr does it (structure checks, duplicates add up, unsorted rows allowed, slots, tail
 * pad), and every one-wave-per-replica CSR form is served: several updates per step (4 | 8, every row length it
 * covers, int8 and bit spins), the narrow int8 and narrow bit-spin forms with every single-site rule, site mode and
 * arithmetic, per-update traces and the pair look-ahead.
 *   Replicas: global replica g belongs to model g / (R_global / n_models); R_global % n_models != 0 is SGA_ERR_INVALID at
 *   sga_init_replicas; with a ladder pass n_ladders = n_models; sga_exchange_pairs takes a pair across models as on
 *   sga_set_dense_shared; sharding through replica0 works, and a shard may begin in the middle of a model.  Model m
 *   walks the chain of a one-model sga_set_csr engine holding (J, h_m) started at replica0 = m * (R_global / n_models),
 *   bit for bit, in whatever form runs: spins, energies, traces, bests, acceptance counters, exchange decisions.
 *   Batch-wide: the accumulation class comes from J alone; accept table, its scale and "covers" come from J and ALL of
 *   H -- row bound max_i (sum_j |J_ij| + max_m |h_mi|), scale 2 as soon as any h_m has a half-integer, no table as soon
 *   as any h_m is off the half-integers (an exact sum stays exact in a wider class, and a table entry stands for the
 *   same dE at any scale: DESIGN.md 4.2d).
 *   sga_get_scan_summary: model 0 only, the 11 CSR words with [2], [6] over all of H.  sga_problem_checksum: the layout
 *   once, all of H, and n_models.  sga_describe: the one-model CSR line with "shared-J models=M"; sga_explain_route the
 *   same from a query with kind = SGA_ROUTE_CSR, n_models = M, shared_j = 1.  Energies, sga_local_fields, sga_flip,
 *   sga_update, export / import (into an engine with the same n_models only), sga_snapshot, stats and timing work.
 *   SGA_ERR_UNSUPPORTED, each message starting "shared-coupling CSR batches": the one-replica-per-workgroup forms, whose
 *   row records carry one field per row -- a problem that fits no one-wave-per-replica form, sga_set_tuning with
 *   waves_per_replica > 1, SGA_CSR_STORAGE_PACKED --, sga_set_field_cache(ON) (AUTO streams), the Wolff rule,
 *   sga_autotune, and a layout that needs 64-bit extents (there is no 64-bit variant).
 *   A NaN or +-Inf in val or H: SGA_ERR_INVALID ("non-finite").  What the caller can get wrong -- extents, a column out
 *   of range, a non-finite value -- is refused BEFORE the engine lets go of the problem it holds: after such a refusal
 *   the previous problem and its replicas are in place.  (A device or memory failure later in the call leaves the engine
 *   without a problem, as the other setters do.)
 *   n_models = 1 is sga_set_csr: same kernels, same sga_describe line. */
int sga_set_csr_shared(sga_engine *e, const int32_t *rowptr, const int32_t *colidx, const float *val,
                       const float *H /* [n_models][n] */, int n, int64_t nnz, int n_models);
/* model m of a ragged batch: its spins and, once replicas exist, its first global replica and replica count */
int sga_get_batch_model(sga_engine *e, int m, int *n_spins, int *first_replica, int *n_replicas);

/* TSP-structured couplings that are never stored (BASELINE configs[4], examples/tsp_example.py
 * at 1000 cities: 10^6 spins whose CSR is 32 GB).  The problem is the one problems/routing.py:250-328
 * compiles, spin (c, p) = city c at tour position p, index c * n_cities + p, in the convention of
 * the build's encoders.tsp_csr:
 *     J[(c,p),(c,p')] = -city_visit/2     J[(c,p),(c',p)] = -position_fill/2
 *     J[(c,p),(c',p-1)] = -dist[c'][c]/4  J[(c,p),(c',p+1)] = -dist[c][c']/4   (c' != c, p mod n)
 * dist: fp32 [n_cities][ld] (host or device; its diagonal is ignored), h: [n_cities^2] fields.
 * The sweep reads two 4 n_cities-byte distance rows per update instead of a 32 n_cities-byte
 * coupling row.  Row sums are exact (checked here) and rounded once to fp32, as in the stored
 * forms, so the chain equals sga_set_csr's on the same couplings bit for bit (production sweeps work
 * on up to eight updates at once, one per wave, wherever they are independent); sga_describe says
 * "acc=f64" without "-exact" in the one case where that cannot be guaranteed (distances spanning
 * more than ~40 binary orders of magnitude).  Single-site flip / update are not available on this
 * form (SGA_ERR_UNSUPPORTED); local fields are. */
int sga_set_tsp(sga_engine *e, const float *dist, int64_t ld, int n_cities, float city_visit,
                float position_fill, const float *h);

/* Couplings that are a sum of complete graphs on groups of sites, never stored (version >= 1000): what
 * encoders.IsingBuilder.add_cardinality_groups builds -- the assignment and scheduling instances, BASELINE
 * configs[1] / configs[3].  Group g is members[member_ptr[g] .. member_ptr[g + 1]) and adds coeff[g] to J_ij for every
 * pair i != j of its members:
 *     J_ij = sum_{g contains i and j} coeff[g]   (i != j),   J_ii = 0
 *     sum_j J_ij s_j = sum_{g contains i} coeff[g] (S_g - s_i),   S_g = sum_{j in g} s_j.
 * A replica keeps its spins as bits and the S_g as integers in LDS: a proposal reads the sums of the site's groups, an
 * accept flips one bit and moves those sums; no coupling is read from HBM.  member_ptr [n_groups + 1], members, coeff
 * [n_groups], h [n]: host or device arrays, not referenced after the call.  Groups of one member and sites in no
 * group are legal (no coupling).
 *   SGA_ERR_INVALID: a member outside [0, n), a site repeated inside one group, extents that are empty, not monotone or
 *   do not start at 0.
 *   SGA_ERR_UNSUPPORTED (sga_last_error says which; sga_set_csr on the materialised couplings serves them all):
 *   - couplings not provably exact in fp32 in any order: every coeff[g] must be an integer multiple of one 2^-k with
 *     2^k max_i sum_{g contains i} |coeff[g]| (|g| - 1) < 2^24 (the bound on sum_j |J_ij| that also bounds every partial
 *     sum the kernel forms).  Under it the row sum equals the stored forms' fp32 row sum bit for bit, so the chain is
 *     sga_set_csr's on the same couplings;
 *   - a site in more than SGA_GROUPS_MAX_MEMBERSHIPS groups;
 *   - spin bits and group sums beyond LDS (160 KiB: about 1.3e6 spins).
 * sga_sweep (every single-site rule, site mode, arithmetic, trace), exchanges, energies, sga_local_fields, best
 * tracking, export / import, the checksum, sga_describe ("groups ... path=groups acc=f32-exact") and the route calls
 * work.  SGA_ERR_UNSUPPORTED: sga_flip, sga_update, the Wolff rule, sga_set_field_cache(ON) (AUTO runs the form as it
 * is), sga_autotune. */
#define SGA_GROUPS_MAX_MEMBERSHIPS 64
int sga_set_groups(sga_engine *e, int n, int n_groups, const int64_t *member_ptr, const int32_t *members,
                   const float *coeff, const float *h);

/* Group couplings plus a stored sparse remainder (version >= 1200): cardinality constraints as groups, the
 * comparatively few explicit pair couplings of the objective (precedence, edge conflicts, flow terms) as a CSR matrix R:
 *     J_ij = sum_{g contains i and j} coeff[g] + R_ij   (i != j),   J_ii = 0
 *     sum_j J_ij s_j = sum_{g contains i} coeff[g] (S_g - s_i) + sum_j R_ij s_j.
 * The constraint part costs no coupling bytes, as in sga_set_groups; R stays in HBM as rptr [n + 1] int32 and (column,
 * value) entries of 8 bytes.  A candidate's remainder row is walked by one lane, once per window; every accept then
 * costs each undecided candidate one binary search (<= 8 probes) in its own row.  rowptr [n + 1], colidx / val [nnz]:
 * host or device arrays, not referenced after the call.  n_groups = 0 with nnz > 0 is legal; nnz = 0 IS sga_set_groups
 * (same kernels, same chain, same sga_describe line).  The group checks are sga_set_groups's.  For R:
 *   SGA_ERR_INVALID: extents that are not monotone or do not span [0, nnz), a column outside [0, n), a value that is
 *   not finite.
 *   SGA_ERR_UNSUPPORTED (sga_last_error names the reason; sga_set_csr on the materialised couplings serves them all):
 *   - a non-zero diagonal entry; R not symmetric; a row not strictly sorted by column (duplicates included);
 *   - a row of more than SGA_GROUPS_MAX_REST_ROW entries (a declared limit of the form: one lane walks a row);
 *   - nnz >= 2^31;
 *   - couplings not provably exact in fp32 in any order: every coeff[g] and every val must be an integer multiple of
 *     one 2^-k with 2^k max_i (sum_{g contains i} |coeff[g]| (|g| - 1) + sum_j |R_ij|) < 2^24.  Under it every partial
 *     sum is exact, the materialised J_ij is itself exact in fp32 and the stored forms' fp32 row sum is the same number:
 *     the chain is sga_set_csr's bit for bit.  A remainder that alone breaks the bound is refused, and so is an
 *     off-grid value (0.1 beside other couplings).
 * Works and is refused as for sga_set_groups; the checksum covers rptr, columns and values; sga_describe reads
 * "groups ... rest_nnz=... rest_max_row=... path=groups acc=f32-exact". */
#define SGA_GROUPS_MAX_REST_ROW 256
int sga_set_groups_csr(sga_engine *e, int n, int n_groups, const int64_t *member_ptr, const int32_t *members,
                       const float *coeff, const int32_t *rowptr, const int32_t *colidx, const float *val,
                       int64_t nnz, const float *h);

/* ---- replicas ------------------------------------------------------------------------- */
/* R_local replicas live on this engine; they are replicas [replica0, replica0+R_local) of a
 * global set of R_global (R_global == R_local, replica0 == 0 on one GPU).  s0 == NULL draws
 * the initial spins from the Philox stream (domain 2), else s0 is int8 +-1 [R_local][n].
 * Energies are computed, best = initial, counters zeroed, sweep counter = 0.  A failed call leaves the
 * engine WITHOUT replicas (the previous set is released first): later sweeps / state calls return
 * SGA_ERR_INVALID until replicas are initialised again. */
int sga_init_replicas(sga_engine *e, int R_local, int R_global, int replica0, uint64_t seed,
                      const int8_t *s0);
/* Temperatures lie in [0, inf].  T = 0 accepts a Metropolis move iff dE <= 0 (a greedy quench: downhill and
 * flat moves), T = inf accepts every Metropolis proposal; every sweep form gives the same chain at both ends, and
 * an exchange whose argument is NaN (two T = 0 slots, a T = 0 slot at equal energies) swaps, as
 * min(1.0, exp(x)) does.  NaN and values with the sign bit set (-0.0 included) are refused with SGA_ERR_INVALID
 * and a message naming the call, before anything changes -- by sga_set_temperatures, sga_set_ladder and the
 * sched argument of sga_sweep, for host-memory inputs (device arrays are not read back to be checked).
 * Temperature of each local replica (used when sga_sweep gets no schedule). */
int sga_set_temperatures(sga_engine *e, const double *T /* [R_local] */);
/* Temperature ladder(s) over the GLOBAL replica set: n_ladders ladders of R_global/n_ladders
 * slots, slot_temps[R_global]; slot i initially holds replica i.  Sets local temperatures. */
int sga_set_ladder(sga_engine *e, const double *slot_temps /* [R_global] */, int n_ladders);

/* ---- hot path ------------------------------------------------------------------------- */
/* n_sweeps Metropolis sweeps (n single-spin updates each) of every local replica.
 *   sched: optional temperatures T(k, r) = sched[k*sched_sweep_stride + r*sched_replica_stride]
 *          (k = sweep within this call, r = local replica), in [0, inf]; NULL = current temperatures.
 *   replay_site [R_local][n_sweeps*n] int32, replay_u [R_local][n_sweeps*n] fp32: SITE_REPLAY
 *          needs both; SITE_SEQUENTIAL takes replay_u if non-NULL (else Philox uniforms).
 *   energy_trace: optional [n_sweeps][R_local] doubles, energy after each sweep.
 *   accept_trace / dE_trace: optional [R_local][n_sweeps*n] per-update records (parity tests).
 */
int sga_sweep(sga_engine *e, int n_sweeps, int site_mode, int arith, const double *sched,
              int64_t sched_sweep_stride, int64_t sched_replica_stride,
              const int32_t *replay_site, const float *replay_u, double *energy_trace,
              uint8_t *accept_trace, double *dE_trace);

/* Single-site operators on local replica r (the reference's per-spin API).
 * sga_local_fields: out[k] = fp32(J[sites[k],:].s) + h[sites[k]] as a double.
 * sga_flip: unconditional flip of `site`; *dE = 2 s_i field; the tracked energy follows.
 * sga_update: one Metropolis update at `site` with uniform u at temperature T. */
int sga_local_fields(sga_engine *e, int r, const int32_t *sites, int count, double *out);
int sga_flip(sga_engine *e, int r, int site, double *dE);
int sga_update(sga_engine *e, int r, int site, double T, float u, int arith, int *accepted,
               double *dE);

/* Rule applied by later sga_sweep / sga_update calls (default METROPOLIS).  GLAUBER and
 * HEAT_BATH always consume the uniform and require SGA_ARITH_F64; the per-update dE record of
 * HEAT_BATH is minus the energy change, as the reference returns it (spin_dynamics.py:188). */
int sga_set_update_rule(sga_engine *e, int rule);
/* SGA_RULE_WOLFF (SpinDynamics._wolff_cluster_dense, core/spin_dynamics.py:210-255; for CSR couplings
 * the same rule over a row's stored entries): a sweep is n cluster moves from drawn start sites,
 * always accepted, n_accepted grows by the cluster sizes, the per-update dE record is
 * compute_energy() after minus before, and energies are evaluated from scratch after every sweep
 * (spin_dynamics.py:87).  Needs SGA_ARITH_F64 and n <= ~31 000 (spins, cluster bitmap and queue in
 * LDS), and CSR rows strictly sorted by column (every stored entry is one bond: duplicates, which the
 * single-site rules add up, are refused with SGA_ERR_UNSUPPORTED); not available for sga_update or
 * sga_set_tsp problems.  One uniform per candidate bond:
 * Philox (domain 3) or, for the parity tests, the recorded stream given here -- u [R_local][capacity]
 * fp32, consumed in draw order by the following Wolff sweeps (NULL: back to Philox). */
int sga_set_wolff_replay(sga_engine *e, const float *u, int64_t capacity);

/* Recompute every local replica's energy from scratch: -0.5 s.(J s) - h.s.  Batches of replicas share
 * one pass over the couplings (EnergyComputer.compute_batch_energies, core/energy_computer.py:142-158):
 * dense problems with >= 32 replicas on the matrix cores, CSR problems with >= 64 replicas through a
 * transposed spin-bit matrix; fewer replicas take one pass each.  E = -1/2 fp32(X) - fp32(Y) with
 * mv_i the fp32 row sum, X = sum_i mv_i s_i and Y = sum_i h_i s_i in fp64 in one order per replica that
 * depends on n alone (blocks of rows, four chains per block, block sums in block order).  Under the
 * default option "batched_energy" = 1 a replica's energy therefore carries the same bits whatever the
 * replica count, the sharding (R_local), this call, sga_init_replicas or sga_set_spins: the batched passes
 * are used only where their row sums and X are the per-replica kernels' bits.  Integer and exactly summable
 * dyadic problems get the exact sums rounded once (mv_i = fp32(S_i), fp32(X), fp32(Y)). */
int sga_recompute_energies(sga_engine *e);

/* One nearest-neighbour replica-exchange round over the ladder(s)
 * (parallel_tempering.py:214-258: even/odd pairs, accept min(1, exp((b_j-b_i)(E_j-E_i)))).
 *   energies_global: [R_global] doubles indexed by GLOBAL replica id (after an all-gather);
 *                    NULL = the engine's own energies: needs R_local == R_global, or every ladder whole
 *                    on one rank (replica0 and R_local multiples of the ladder length) -- then only the
 *                    local ladders are decided (same Philox keys as in the unsharded run: global ladder
 *                    index), the slot map / exchange statistics of the other ranks' ladders stay
 *                    untouched here, and *n_accepted counts the local ladders' swaps.
 *   start: [n_ladders] int32 0/1 parity per ladder, NULL = Philox (domain 1).
 *   u: [n_ladders][slots/2] doubles in attempt order, NULL = Philox.
 *   n_accepted: optional out (host int). */
int sga_exchange(sga_engine *e, const double *energies_global, const int32_t *start,
                 const double *u, int *n_accepted);

/* Exchange attempts over an ordered list of slot pairs: the CPU branch of the reference's
 * exchange_method="all_pairs" (annealing/parallel_tempering.py:222-232 -- for i < j, gated by
 * `np.random.rand() < 0.1`, _attempt_single_exchange(i, j), :234-258; statistics under
 * min(i, j)).  Each attempt sees the swaps before it.  pairs: host [count][2] int32 global
 * slot indices in attempt order (the gate is the caller's: it only selects the list);
 * u: [count] doubles or NULL (Philox, domain 1); energies_global as in sga_exchange. */
int sga_exchange_pairs(sga_engine *e, const double *energies_global, const int32_t *pairs,
                       const double *u, int count, int *n_accepted);

/* ---- isoenergetic cluster moves (version >= 2500; csrc/cluster_moves.hip) ------------------------------------------
 * The cluster move of parallel tempering on frustrated sparse couplings (Houdayer 2001; Zhu, Ochoa and Katzgraber 2015)
 * between two replicas a, b of ONE Hamiltonian: the sites where the two differ; one of them drawn uniformly; the
 * connected component of differing sites around it, connected through stored non-zero couplings (an entry whose value
 * is +-0 connects nothing); that component flipped in both replicas.  On the component the move swaps the two
 * configurations and every coupling that leaves it ends on a site where the replicas agree, so E_a + E_b is conserved
 * exactly for any J and h: the move is rejection free.  Identical replicas: nothing happens (size 0).
 *   EQUAL TEMPERATURES WITHIN A PAIR ARE THE CALLER'S RESPONSIBILITY: only there is the move a valid Monte-Carlo step.
 *   The pair form does not look at temperatures; the ladder form pairs equal slot indices of two ladders, which hold
 *   equal temperatures where the ladders were set up with the same temperatures (sga_set_ladder of a tiled ladder).
 *   The draw: Philox4x32-10, key = the engine's seed, counter (0, round, min(global id of a, global id of b), 5),
 *   global id = replica0 + local index; with count = the number of differing sites the seed site is the
 *   ((word 0 * count) >> 32)-th of them in index order.  round is the caller's: no counter of the engine moves.
 *   Served: one-model CSR problems (sga_set_csr, sga_set_csr64, a sparse matrix that sga_set_dense kept as CSR) and
 *   sga_set_csr_shared, where both replicas of a pair must lie under the same field vector (SGA_ERR_INVALID otherwise).
 *   SGA_ERR_UNSUPPORTED, with the reason in sga_last_error: dense couplings (every differing site is connected to every
 *   other: the component is always all of them, the move a plain exchange of the two replicas), sga_set_tsp, sga_set_groups
 *   and sga_set_groups_csr (no stored rows to walk), ragged batches, n beyond what the kernel's bitmaps hold in LDS
 *   (n / 2 bytes of the 160 KiB: n <= 327 040).
 *   SGA_ERR_INVALID: a NULL engine or pair list; no problem or no replicas; count < 0; an index outside [0, R_local); a
 *   replica named twice, or a == b; the ladder form: no ladder, an odd n_ladders, R_local != R_global, a slot range not
 *   inside [0, slots).  count == 0 and an empty slot range are no-ops.  Every refusal happens before anything is
 *   enqueued or changed.
 *   After the call, enqueued on the engine's stream behind earlier sweeps: the spins of the replicas whose cluster was
 *   not empty are flipped there; their tracked energies are what sga_recompute_energies would store, bit for bit; the
 *   best of each follows where the new energy is lower (the step a sweep's end runs); their accept counters grow by
 *   the cluster's size (as under SGA_RULE_WOLFF); the cached local fields are seeded again by the next sweep (as after
 *   sga_set_spins).  Every other replica, the temperatures, the slot map, the exchange statistics and the sweep / round
 *   counters are unchanged.  Cost beside the move itself: one from-scratch energy pass over the local replicas.
 *   sizes: the clusters' sizes, host or device, or NULL.  A device buffer: the call returns at once; a host buffer:
 *   after the copy has landed. */
/* pairs: host [count][2] int32 LOCAL replica indices, every replica at most once, a != b */
int sga_cluster_move_pairs(sga_engine *e, const int32_t *pairs, int count, uint32_t round,
                           int32_t *sizes /* [count], host or device, or NULL */);
/* ladders 2c and 2c+1, slots slot_lo <= s < slot_hi: the replicas that hold slot s of both, read
 * from the slot map ON THE DEVICE (no host round trip); needs an even n_ladders and R_local == R_global */
int sga_cluster_move_ladders(sga_engine *e, int slot_lo, int slot_hi, uint32_t round,
                             int32_t *sizes /* [n_ladders/2][slot_hi - slot_lo] or NULL */);

/* ---- population annealing: the resampling step (version >= 2600; csrc/resample.hip) --------------------------------
 * Population annealing (Hukushima and Iba 2003; Machta 2010; Wang, Machta and Katzgraber 2015) cools a population of
 * replicas together; between two temperatures every replica is copied or culled in proportion to exp(-(beta' - beta) E).
 * This call is that step, on the device and exact in integers, so that it is a function of the tracked energies, dbeta,
 * the engine's seed and `round` alone.  The local replicas are cut into n_populations contiguous blocks of
 * N = R_local / n_populations members; for population p with members r = 0 ... N - 1:
 *   x_r = (-dbeta[p]) * E_r (one fp64 product), x_max = max_r x_r, W_r = (uint64)(exp(x_r - x_max) * 2^40), exp the
 *   deterministic fp64 exp of the sweeps' accept rule; the product is exact, the cast truncates, exp(0) is exactly 1, so
 *   S = sum W_r >= 2^40, and N <= 2^23 keeps S < 2^64.  C_r = W_0 + ... + W_r.
 *   The draw: Philox4x32-10, key = the engine's seed, counter (0, round, replica0 / N + p, 6): U = (word 0 << 32) | word 1,
 *   the offset o = (U * S) >> 64, 0 <= o < S.
 *   Systematic resampling: child k = 0 ... N - 1 sits at t_k = k S + o and its parent is the r with
 *   N C_{r-1} <= t_k < N C_r (128-bit integer compares).  n_r, the children of r, is the floor or the ceiling of
 *   N W_r / S, and sum n_r = N.
 *   Placement: every r with n_r >= 1 keeps its slot; the slots with n_r == 0, in ascending order, receive the surplus
 *   copies in ascending order (parent r repeated n_r - 1 times, ascending in r).  A source is never a destination.
 *   The relative weight lost to the truncation of W_r is below N * 2^-40.
 *   dbeta: host [n_populations], finite.  round is the caller's: no counter of the engine moves.
 *   parents: [R_local] the LOCAL index of every slot's parent (d itself where the slot is not overwritten); shift:
 *   [n_populations] x_max; weight_sum: [n_populations] S.  ln Q_p = shift[p] + ln(weight_sum[p] / (N * 2^40)) is the
 *   free-energy increment of the step; the logarithm is the caller's, so both outputs are exact.  Each of the three is a
 *   host or a device buffer or NULL.  The work is enqueued on the engine's stream behind earlier sweeps; with device
 *   outputs only the call returns at once, with a host output after its copy has landed.
 *   After the call, an overwritten slot holds its parent's spins and tracked energy (the parent's bits: no energy pass
 *   runs); its best becomes the parent's current state where the parent's energy is below the slot's best, else it is
 *   kept (the best over all replicas is never lost); its accept counter is unchanged.  The cached local fields are seeded
 *   again by the next sweep (as after sga_set_spins).  Every surviving slot, the temperatures (the new ones are the
 *   caller's to set), the slot map, the exchange statistics, the sweep / round counters and the Wolff cursors are unchanged.
 *   Served: every kind of problem.  Batches (sga_set_dense_batch, sga_set_dense_shared, sga_set_csr_batch,
 *   sga_set_csr_shared) where no population spans two models; shards where replica0 and R_local are multiples of N.
 *   SGA_ERR_INVALID, before anything is enqueued or changed: a NULL engine or dbeta; no problem or no replicas;
 *   n_populations < 1 or not a divisor of R_local; N > 2^23; a dbeta that is NaN or infinite; a device dbeta; a
 *   population across two models; a shard boundary inside a population. */
int sga_resample(sga_engine *e, int n_populations, const double *dbeta /* host [n_populations] */, uint32_t round,
                 int32_t *parents   /* [R_local] local indices, host or device, or NULL */,
                 double *shift      /* [n_populations] x_max, host or device, or NULL */,
                 uint64_t *weight_sum /* [n_populations] S, host or device, or NULL */);

/* ---- spin and link overlaps between pairs of replicas (version >= 2700; csrc/pair_overlaps.hip) ----------------------
 * What a sampler with two copies of a ladder measures per temperature -- P(q), <q^2>, the Binder ratio, the link overlap
 * q_l -- as exact integer counts formed where the spins are.  For a pair (a, b) of local replicas let
 * x_i = [s_a[i] != s_b[i]] for the sites i < n:
 *   d = sum_i x_i, the distance: n q_ab = n - 2 d (int32).
 *   A LINK is an entry (i, j) of the engine's packed rows whose value is not +-0, with j != i and 0 <= j < n: the entries
 *   the isoenergetic cluster move connects through.  Padding of long-row layouts and stored zeros are none; a stored
 *   diagonal entry is none; both triangles count as they are stored (a symmetric matrix has every bond twice).  Packing
 *   keeps every input entry as it came ("duplicates add up" in a row sum, they are not merged): a duplicate (i, j) is
 *   TWO links.  L = the number of links, a constant of the problem (sga_get_link_count; int64: a graph may hold more
 *   than 2^31 entries).
 *   b = the number of links with x_i != x_j, the broken links: L q_l = L - 2 b (int64).
 *   The pair form takes any list of pairs: the call only reads, so a replica may stand in many pairs, and a == b is a
 *   pair (d = b = 0).  dist and broken: host or device, one of them may be NULL.
 *   The ladder form takes the pairs of sga_cluster_move_ladders: ladders 2c and 2c + 1, slots slot_lo <= s < slot_hi, the
 *   replicas that hold them read from the slot map ON THE DEVICE; it needs an even n_ladders and R_local == R_global.
 *   The cell of pair c and slot s is k = c (slot_hi - slot_lo) + (s - slot_lo); the call adds exactly 1 to
 *   hist_q[k bins_q + min(d >> q_shift, bins_q - 1)] and, where hist_l is given, to
 *   hist_l[k bins_l + min(b >> l_shift, bins_l - 1)].  The clamp keeps the store inside the cell for any bin count; the
 *   exact layout is shift 0 with n + 1 (L + 1) bins.  The histograms are the CALLER'S DEVICE BUFFERS, [cells][bins]
 *   uint64, zeroed by the caller once: the engine keeps nothing between calls and never zeroes them; one workgroup owns
 *   one cell per launch, so the count is a plain load / add / store, deterministic.
 *   Served -- d: every kind of problem (ragged batches: rows are zero past a model's own sites and never differ there).
 *   b, hist_l and sga_get_link_count: the problems the cluster move serves -- one-model CSR (sga_set_csr, sga_set_csr64,
 *   a sparse matrix that sga_set_dense kept as CSR) and sga_set_csr_shared, where a pair under two field vectors is
 *   served too (the graph is one).  SGA_ERR_UNSUPPORTED, with the reason in sga_last_error: a non-NULL broken or hist_l,
 *   or sga_get_link_count, on dense couplings, sga_set_tsp, sga_set_groups / sga_set_groups_csr or ragged batches; links
 *   with n beyond the kernel's bitmap of differing sites in LDS (n / 8 bytes of the 160 KiB: n <= 1 308 160).  Without
 *   links no bitmap is built and no bound on n applies.
 *   SGA_ERR_INVALID: a NULL engine; no problem or no replicas; which outside {SGA_SPINS_CURRENT, SGA_SPINS_BEST};
 *   count < 0, or a NULL pair list with count > 0; a pair list on the device; an index outside [0, R_local); dist and
 *   broken both NULL; a NULL n_links; bins < 1; a shift outside [0, 31]; a NULL or host hist_q, a host hist_l; no ladder,
 *   an odd n_ladders, R_local != R_global, a slot range not inside [0, slots).  count == 0 and an empty slot range are
 *   no-ops.  Every refusal happens before anything is enqueued or written.
 *   Read only: no spin, energy, best, counter, cached field, window plan, slot map or sga_get_last_kernel changes, and a
 *   run with these calls between its sweeps walks the same chain.  The work is enqueued on the engine's stream behind
 *   earlier sweeps; with device outputs the call returns at once, with a host output after its copy has landed. */
int sga_get_link_count(sga_engine *e, int64_t *n_links /* host or device */);
/* pairs: host [count][2] int32 LOCAL replica indices */
int sga_get_pair_overlaps(sga_engine *e, int which /* SGA_SPINS_CURRENT | SGA_SPINS_BEST */,
                          const int32_t *pairs /* host [count][2], LOCAL indices */, int count,
                          int32_t *dist /* [count], host or device, or NULL */,
                          int64_t *broken /* [count], host or device, or NULL */);
/* the CURRENT spins; hist_q [n_ladders/2][slot_hi - slot_lo][bins_q], hist_l [...][bins_l]: device, uint64 */
int sga_accumulate_ladder_overlaps(sga_engine *e, int slot_lo, int slot_hi,
                                   uint64_t *hist_q, int bins_q, int q_shift,
                                   uint64_t *hist_l /* or NULL */, int bins_l, int l_shift);

/* ---- class-resolved overlaps between pairs of replicas (version >= 2800; csrc/class_overlaps.hip) --------------------
 * The overlap between two replicas resolved by a CLASS of sites -- the planes of a lattice, sublattices, layers,
 * communities, the machines of a scheduling instance -- as exact integer counts formed where the spins are: what the
 * wave-vector-dependent spin-glass susceptibility chi_SG(k) and the correlation length xi_L / L are made of.
 *   A CLASS MAP is classes[m][i]: int32, n_maps rows with leading dimension ld >= n, values in [0, n_classes).  A site
 *   whose value lies outside that range, negative included, belongs to NO class in that map: that is how callers mask
 *   sites, and the kernel tests the range and never trusts it, so a map the host never saw cannot index out of bounds.
 *   For a pair (a, b) of local replicas let x_i = [s_a[i] != s_b[i]] for the sites i < n:
 *   D[m][c] = sum_{i : classes[m][i] = c} x_i (int32).  With N_c the size of the class, the class overlap is
 *   Q_c = N_c - 2 D_c; where a map gives every site a class, sum_c D[m][c] = d of sga_get_pair_overlaps.
 *   The pair form takes `which` and a host pair list under the rules of sga_get_pair_overlaps: any list, a replica may
 *   stand in many pairs, a == b is a pair and gives all zeros.  classes: a host or a device buffer; a HOST MAP IS
 *   STAGED ON EVERY CALL (4 n_maps n bytes over the bus) -- a run keeps its map on the device.  dist:
 *   [count][n_maps][n_classes] int32, host or device; a device output returns at once, a host output after its copy has
 *   landed.
 *   The ladder form takes the pairs of sga_accumulate_ladder_overlaps: ladders 2c and 2c + 1, slots
 *   slot_lo <= s < slot_hi, the replicas that hold them read from the slot map ON THE DEVICE; it needs an even
 *   n_ladders and R_local == R_global.  The cell of pair c and slot s is k = c (slot_hi - slot_lo) + (s - slot_lo).
 *   Each call adds D[m][c] to sum1[k][m][c] and, where sum2 is not NULL, D[m][c] D[m][c'] to sum2[k][m][c][c'], the full
 *   C x C matrix for every c, c'.  classes, sum1 and sum2 are the CALLER'S DEVICE BUFFERS, the sums uint64, zeroed by
 *   the caller once: the engine keeps nothing between calls and never zeroes them; one workgroup owns one cell per
 *   launch, so the update is a plain 64-bit load / add / store, deterministic, no atomics on global memory.  The caller
 *   counts its own calls: each adds one measurement to every cell of the range.  From these sums every second moment
 *   follows in exact integers, <Q_c Q_c'> = N_c N_c' - 2 N_c <D_c'> - 2 N_c' <D_c> + 4 <D_c D_c'>, and any wave vector
 *   afterwards on the host.  Overflow is the caller's to respect: measurements (max_c N_c)^2 < 2^64.
 *   Served: every kind of problem, as d of sga_get_pair_overlaps -- only the int8 spin rows are read; n is the engine's
 *   row length in sites (ragged batches: rows are zero past a model's own sites and never differ there).
 *   The kernel (one workgroup of 256 threads per pair) keeps a counter per (m, c) in LDS, a copy for each of its four
 *   waves where n_maps n_classes <= 10 224, one copy up to 40 896: 4 bytes x copies x n_maps n_classes of LDS.
 *   SGA_ERR_UNSUPPORTED, with the reason in sga_last_error: n_maps n_classes > 40 896.
 *   SGA_ERR_INVALID: a NULL engine, classes or output; no problem or no replicas; which outside {SGA_SPINS_CURRENT,
 *   SGA_SPINS_BEST}; every pair-list error of sga_get_pair_overlaps; n_maps < 1, n_classes < 1 or ld < n; a host sum1,
 *   sum2 or classes in the ladder form; no ladder, an odd n_ladders, R_local != R_global, a slot range not inside
 *   [0, slots).  count == 0 and an empty slot range are no-ops.  Every refusal happens before anything is enqueued or
 *   written.
 *   Read only: no spin, energy, best, counter, cached field, window plan, slot map or sga_get_last_kernel changes, and a
 *   run with these calls between its sweeps walks the same chain.  The work is enqueued on the engine's stream behind
 *   earlier sweeps. */
int sga_get_class_overlaps(sga_engine *e, int which /* SGA_SPINS_CURRENT | SGA_SPINS_BEST */,
                           const int32_t *pairs /* host [count][2], LOCAL indices */, int count,
                           const int32_t *classes /* [n_maps][ld], host or device */, int64_t ld, int n_maps, int n_classes,
                           int32_t *dist /* [count][n_maps][n_classes], host or device */);
/* the CURRENT spins; sum1 [n_ladders/2][slot_hi - slot_lo][n_maps][n_classes], sum2 [...][n_classes][n_classes]: device, uint64 */
int sga_accumulate_ladder_class_overlaps(sga_engine *e, int slot_lo, int slot_hi,
                                         const int32_t *classes /* [n_maps][ld], device */, int64_t ld, int n_maps, int n_classes,
                                         uint64_t *sum1, uint64_t *sum2 /* or NULL */);

/* ---- simulated quantum annealing: Trotter slices coupled in the sweep (version >= 2900; csrc/sweep_transverse.hip) ---
 * Path-integral Monte Carlo of the transverse-field Ising model: P replicas -- the Trotter slices of ONE instance -- each
 * sweep under a field that depends on the spins of the two neighbouring slices.
 *   The local replicas are cut into G = R_local / P contiguous groups of P = n_slices slices; each group is one instance
 *   of the quantum problem.  replica0 % P == 0, so groups lie whole on a rank and no collective is needed.  The slice
 *   index of local replica r is p = (replica0 + r) % P, its neighbours are the slices p +- 1 mod P of its group (P = 2:
 *   both neighbours are the same slice, counted twice).
 *   Sweep kk of the call is two half-sweeps, enqueued on the engine's stream: half-sweep A moves the slices with even p
 *   while the odd ones stand still, half-sweep B the odd ones.  P is even, so a moving slice never has a moving neighbour.
 *   Within a half-sweep every moving slice r performs the n updates t = 0 ... n-1 of sga_sweep's production stream in
 *   SGA_SITE_RANDOM mode: site and u from Philox counter (t >> 1, sweeps_done + kk, replica0 + r, 0) -- domain 0, no new
 *   domain word.  The update at site i:
 *     a     = s_up[i] + s_dn[i] in {-2, 0, 2}, the neighbour slices as they stand at the start of the half-sweep;
 *     h_eff = h_i + k (float)a in fp32, k = k_perp[kk][g] (the product is exact: the sum rounds once, an FMA gives the
 *             same bits);
 *     the decision is the engine's Metropolis rule in `arith` on (fp32 row sum of J s, s_i, h_eff, T_r, u): what
 *             sga_update decides for a problem whose field at i is h_eff, T = 0 and T = inf included;
 *     on accept the spin flips, the accept counter grows by one and the tracked energy moves by the CLASSICAL dE -- the
 *             dE the same rule computes with h_i in place of h_eff, what sga_flip would report: the tracked energy stays
 *             the slice's classical energy -1/2 s J s - h s (sga_recompute_energies gives the same value).
 *   After both half-sweeps of a sweep every slice's best follows where its energy is lower (the step a sweep's end runs).
 *   sweeps_done grows by n_sweeps at the end of the call; the cached local fields are marked for re-seeding, as after
 *   sga_set_spins.  Temperatures, the slot map, exchange statistics, round counters and Wolff cursors do not move.
 *   By construction: with k = 0 everywhere the call is sga_sweep(n_sweeps, SGA_SITE_RANDOM, arith) bit for bit (spins,
 *   energies, bests, counters), and a call of 2 sweeps equals two calls of 1 sweep.
 *   Equal temperatures within a group are the caller's responsibility, as with the cluster move.  So is the physical
 *   mapping: at temperature T and transverse field Gamma each slice runs at P T with
 *   k_perp = -(P T / 2) ln tanh(Gamma / (P T)) in classical energy units.  Any finite k_perp, negative values included.
 *   k_perp is a HOST array, copied to the device once per call (it has left the caller's buffer on return).
 *   Served: one-model CSR problems (sga_set_csr, sga_set_csr64, a sparse matrix that sga_set_dense kept as CSR) whose
 *   set-time class has an exact fp32 integer row sum in any order (integer J; any fp32 h), symmetric with a zero
 *   diagonal, under SGA_RULE_METROPOLIS, a slice's int8 spins within LDS (n <= ~163 000).
 *   SGA_ERR_UNSUPPORTED, with the reason in sga_last_error: dense couplings, sga_set_tsp, sga_set_groups /
 *   sga_set_groups_csr, batches (ragged and shared), the other CSR classes (real-valued J needs the canonical order),
 *   rules other than Metropolis, asymmetric J or a non-zero diagonal.
 *   SGA_ERR_INVALID, before anything is enqueued or changed: a NULL engine or k_perp, a device k_perp; no problem or no
 *   replicas; n_sweeps < 0; a bad arith; P odd, P < 2, P not a divisor of R_local, replica0 % P != 0; a NaN or infinite
 *   k_perp.  Argument errors are reported before the problem's kind is looked at.  n_sweeps == 0 is a no-op.
 *   The launches (two per sweep, built per arithmetic) show in sga_get_last_kernel; sga_enable_timing does not bracket them. */
int sga_sweep_transverse(sga_engine *e, int n_sweeps, int n_slices, int arith /* SGA_ARITH_* */,
                         const float *k_perp /* host [n_sweeps][R_local / n_slices] */);

/* ---- simulated quantum annealing on dense couplings (version >= 3100; csrc/sweep_transverse_clf.hip, _fx.hip) ----------
 * The step of sga_sweep_transverse, word for word -- groups, half-sweeps, the production stream, h_eff = h_i + k (float)a
 * in fp32, the Metropolis rule in `arith`, the classical dE on accept, bests after the sweep, counters -- on ONE dense
 * matrix, in the form of the cached-local-field sweep: a moving slice keeps F = scale (J s + h) in LDS and reads a
 * coupling row only when a proposal is accepted.  The rule sees the exact integer row sum dot_i = (F_i - scale h_i) /
 * scale and h_eff: (double)dot + (double)h_eff under SGA_ARITH_F64, that sum rounded to fp32 once under SGA_ARITH_F32.
 *   By construction: with k = 0 everywhere the call is sga_sweep(n_sweeps, SGA_SITE_RANDOM, arith) bit for bit, a call of 2
 *   sweeps equals two calls of 1, and the same integer couplings held as CSR under sga_sweep_transverse give the same chain.
 *   Fields.  The call seeds the resident fields where they are not valid (the pass the cached sga_sweep uses) and keeps
 *   them valid: every launch writes the moving slices' fields back, and a cached sga_sweep after it goes on without
 *   seeding.  (Under SGA_FIELD_CACHE_AUTO, which routes replica by replica, the call seeds them every time.)  The field
 *   cache mode itself is not looked at: the call is its own opt-in.
 *   Served: one dense model (sga_set_dense) that the integer cached-field form admits -- integer symmetric J with a zero
 *   diagonal, h in multiples of 1/2, row bound below 2^24; int8 and fp32 rows, int16 and int32 fields -- under
 *   SGA_RULE_METROPOLIS, with a slice's fields, spin bits, two rows of neighbour bits and decision slots within LDS
 *   (163 584 bytes): 2.375 n + 512 bytes with int16 fields, 4.375 n + 512 with int32 fields, rows padded to 128 elements:
 *   n <= 68 608 and n <= 37 248.  Option "clf_waves" sets the waves per slice; 0 leaves the cached sweep's choice, taken
 *   over the R_local / 2 workgroups of a launch.
 *   Fixed-point fields (version >= 3400; csrc/sweep_transverse_fx.hip).  With option "clf_fixed_point" = 1 set before
 *   sga_set_dense, a dense model the integer form does not take is served on the fixed-point cached fields instead: J in
 *   one of the exact accumulation classes (integer J; J on a binary grid 2^-k, such as half- and quarter-valued penalty
 *   encodings), symmetric with a zero diagonal, ANY fp32 h.  D = 2^k J s is kept exactly as int32 | int64 in LDS, h is
 *   never folded in; the rule sees dot = fp32(2^-k D_i) -- the row kernels' dot, one rounding of the exact row sum --
 *   and h_eff: metropolis on (dot, s_i, h_eff) in `arith`, exactly the classical fixed-point sweep's call with h_eff in
 *   place of h_i; on accept E moves by that call's dE for h_i.  Everything said above holds: k = 0 is sga_sweep bit for
 *   bit, the fields stay valid for the cached sga_sweep and are traded by sga_exchange_transverse.  LDS: 4.375 n + 512
 *   bytes with int32 fields (n <= 37 248), 8.375 n + 512 with int64 fields (n <= 19 456).  A problem the integer form
 *   takes keeps the integer kernel whatever the option says; with the option at 0 nothing changes.
 *   SGA_ERR_INVALID, first and with the engine unchanged: exactly what sga_sweep_transverse reports so, in the same words.
 *   SGA_ERR_UNSUPPORTED, with the reason in sga_last_error: sga_set_tsp, sga_set_groups / sga_set_groups_csr, batches
 *   (ragged, shared and stacked), CSR engines -- a sparse matrix that sga_set_dense kept as CSR included: they are
 *   sga_sweep_transverse's --, a dense problem the integer cached-field form does not take (real-valued J, a non-zero
 *   diagonal, asymmetric J, a bound of 2^24 or more: the set-time scan's reason) unless the fixed-point form serves it,
 *   and under option "clf_fixed_point" a problem that form refuses too (J that needs the canonical fp64 order, asymmetric
 *   J, a diagonal, fields wider than int64: the fixed-point verdict's reason), rules other than Metropolis, a slice beyond
 *   LDS.  World-line clusters on dense couplings are sga_worldline_clusters_dense's; it does not serve fixed-point fields.
 *   The launches (two per sweep) show in sga_get_last_kernel; sga_enable_timing does not bracket them. */
int sga_sweep_transverse_dense(sga_engine *e, int n_sweeps, int n_slices, int arith /* SGA_ARITH_* */,
                               const float *k_perp /* host [n_sweeps][R_local / n_slices] */);

/* ---- world-line cluster updates for simulated quantum annealing (version >= 3000; csrc/worldline_clusters.hip) --------
 * Swendsen-Wang clusters along the imaginary-time direction at one site, flipped under the classical field (Rieger and
 * Kawashima 1999; Heim et al. 2015): what keeps simulated quantum annealing ergodic at small Gamma, where k_perp freezes
 * the slices of sga_sweep_transverse into identical copies.
 *   Groups.  Those of sga_sweep_transverse: G = R_local / P contiguous groups of P = n_slices slices, replica0 % P == 0.
 *   Slice p of group g is local replica g P + p with global id q_p = replica0 + g P + p.  T_g is the temperature of
 *   local replica g P; equal temperatures within a group are the caller's responsibility, as there.  2 <= P <= 64; P
 *   need not be even.
 *   Threshold.  thr = (uint32_t)floor(p_bond[kk][g] * 16777216.0), formed on the host in double; p = 1 gives 2^24: every
 *   bond between equal spins is active.
 *   Order.  For sweep kk = 0 ... n_sweeps-1 the sites go in typewriter order i = 0 ... n-1; at each site all of the
 *   following is decided from the spins as they stand when the site is reached.
 *     1. Draws.  Each slice p takes ONE Philox block at counter (i, (uint32_t)(round + kk), q_p, 4), the engine's 64-bit
 *        seed as key.  Domain word 4 is DOMAIN_WORLDLINE = sweep | 1 << 2 (in use besides: 0, 1, 2, 5, 6; every Wolff
 *        word ends in bits 11).  Word 0 decides the bond from slice p to slice (p+1) mod P:
 *          b_p = (s_p[i] == s_{p+1}[i]) && ((w0 >> 8) < thr).
 *        Word 1 gives u_p = (w1 >> 8) 2^-24 as fp32.  For P = 2 the two bonds join the same pair and both are drawn:
 *        the doubled coupling the transverse sweep uses there.
 *     2. Segments.  Slice p is a head iff b_{(p-1) mod P} is false.  With no head the whole ring is one segment with
 *        head 0; otherwise each head f owns f, f+1, ... cyclically up to the slice before the next head.
 *     3. Decision per segment with head f, size m and common spin sigma = s_f[i]:
 *          A   = sum over the segment of dot_p, dot_p = sum_j J_ij s_p[j]: an exact integer, |A| < 2^30 by the admitted
 *                class, accumulated in int32;
 *          Phi = (double)A + (double)m * (double)h_i (the product is exact, the sum rounds once);
 *          dE  = 2 sigma Phi;
 *          flip iff dE <= 0 or (double)u_f < (double)expf((float)(-dE / T_g)): the fp64 Metropolis rule of the oracle
 *          (metropolis_core, SGO_ARITH_F64); T = 0 and T = inf behave as that expression does.  There is no `arith`
 *          argument: only this rule is built, whatever sga_set_update_rule says.
 *     4. On a flip every slice of the segment takes -sigma at site i, and its tracked energy moves by
 *        2 sigma ((double)dot_p + (double)h_i) -- what sga_flip reports: the tracked energies stay classical and equal
 *        sga_recompute_energies.
 *   After the n sites of a sweep every slice's best follows where its energy is lower (the step a sweep's end runs).
 *   What does not move: sweeps_done, the exchange round counters, accept counters, temperatures, the slot map, exchange
 *   statistics and Wolff cursors.  `round` is the caller's, as with sga_cluster_move_pairs.  The cached local fields are
 *   marked for re-seeding, as after sga_set_spins.
 *   By construction a call of 2 sweeps at `round` equals a call of 1 at `round` followed by a call of 1 at `round + 1`;
 *   n_sweeps == 0 is a no-op.
 *   With p_bond = 1 - exp(-2 k_perp / T_g) one site update satisfies detailed balance against exp(-H_eff / T_g), H_eff
 *   the effective energy of the transverse sweep at k_perp.
 *   p_bond is a HOST array (it has left the caller's buffer on return); stats, where given, is a HOST array the call adds
 *   to and waits for: per group the segments formed, the segments flipped and the slice spins flipped.
 *   SGA_ERR_INVALID, first and with the engine unchanged: a NULL engine or p_bond, a device p_bond or stats; no problem or
 *   no replicas; n_sweeps < 0; P < 2, P > 64, P not a divisor of R_local, replica0 % P != 0; a p_bond that is NaN or
 *   outside [0, 1].
 *   SGA_ERR_UNSUPPORTED, with the reason in sga_last_error: everything sga_sweep_transverse refuses, for the same reasons,
 *   except the update rule, which this call ignores; and a group's spin words beyond LDS (one word of 4 bytes per site
 *   for P <= 32, of 8 bytes beyond: n <= ~40 000 and ~20 000).
 *   The launch (one per call) shows in sga_get_last_kernel; sga_enable_timing does not bracket it. */
int sga_worldline_clusters(sga_engine *e, int n_sweeps, int n_slices, uint32_t round,
                           const double *p_bond /* host [n_sweeps][R_local / n_slices], each in [0, 1] */,
                           int64_t *stats       /* host [R_local / n_slices][3] or NULL: += segments formed, segments flipped, slice spins flipped */);

/* ---- world-line cluster updates on dense couplings (version >= 3200; csrc/worldline_clusters_dense.hip) ----------------
 * The step of sga_worldline_clusters, word for word as stated above -- groups, 2 <= P <= 64, thresholds, typewriter order,
 * one Philox block per slice and site at (i, round + kk, q_p, 4), segments from the bonds, A in int32, the fp64 Metropolis
 * rule with the head's uniform at T_g whatever the engine's rule, the tracked energy of a flipped slice moved by
 * 2 sigma ((double)dot_p + (double)h_i), bests after the n sites of each sweep, 2 sweeps at `round` = 1 + 1, n_sweeps == 0 a
 * no-op, no counter, temperature, slot map or statistic moved -- on ONE dense matrix.  The row sum is read from the resident
 * fields F = scale (J s + h) of the cached-local-field sweep, dot_p = (F_p[i] - scale h_i) / scale, an exact integer: a
 * coupling row is read only for a site where a segment flips.  By construction the same integer couplings held as CSR
 * under sga_worldline_clusters walk the same chain bit for bit.
 *   The differences:
 *   Fields.  The cached local fields are NOT marked for re-seeding.  The call seeds them where they are not valid (the pass
 *   the cached sga_sweep uses; under SGA_FIELD_CACHE_AUTO every time, as sga_sweep_transverse_dense does), updates them for
 *   every flip and leaves them valid: sga_sweep_transverse_dense, this call, sga_sweep_transverse_dense run without seeding
 *   in between.  A launch that did not go out leaves them marked for re-seeding.  The field cache mode itself is not
 *   looked at: the call is its own opt-in.
 *   Served: one dense model (sga_set_dense) that the integer cached-field form admits -- integer symmetric J with a zero
 *   diagonal, h in multiples of 1/2, row bound below 2^24 (so |dot| < 2^24 and |A| < 2^30 at P = 64); int8 and fp32 rows,
 *   int16 and int32 fields.  The kernel keeps nothing of size n in LDS (the fields stay in HBM / L2): no bound on n beyond
 *   the memory of the fields.  Option "clf_waves" sets the waves per group; 0 leaves one wave per 1-KiB chunk of a row,
 *   eight at the most.
 *   SGA_ERR_INVALID, first and with the engine unchanged: exactly what sga_worldline_clusters reports so, in the same words.
 *   SGA_ERR_UNSUPPORTED, with the reason in sga_last_error: sga_set_tsp, sga_set_groups / sga_set_groups_csr, batches
 *   (ragged, shared and stacked), CSR engines -- a sparse matrix that sga_set_dense kept as CSR included: they are
 *   sga_worldline_clusters' --, a dense problem the integer cached-field form does not take (the set-time scan's reason),
 *   fields of another width (the fixed-point forms).  The update rule is not looked at.
 *   The launch (one per call) shows in sga_get_last_kernel; sga_enable_timing does not bracket it. */
int sga_worldline_clusters_dense(sga_engine *e, int n_sweeps, int n_slices, uint32_t round,
                                 const double *p_bond /* host [n_sweeps][R_local / n_slices], each in [0, 1] */,
                                 int64_t *stats       /* host [R_local / n_slices][3] or NULL: += as sga_worldline_clusters */);

/* ---- time links and the exchange along the transverse field (version >= 3300; csrc/trotter_exchange.hip) ------------------
 * Groups as in sga_sweep_transverse: G = R_local / n_slices groups of P = n_slices slices, slice p of group g in row g P + p,
 * the slices of a group a ring.  The BROKEN TIME LINKS of group g over the current spins are
 *   B_g = sum_{p < P} sum_{i < n} [ s_{gP+p}[i] != s_{gP+next(p)}[i] ],   next(p) = p + 1 == P ? 0 : p + 1,
 * so with P = 2 both links of the ring count and a differing site gives 2, as the sweep counts its neighbour twice; B is
 * even and lies in [0, n P].  B is all of a configuration that the quantum side reads: <sigma^x> and the quantum energy
 * estimator are functions of it (quantum.transverse_magnetization, quantum.quantum_energy), and so is the acceptance ratio
 * of an exchange between two groups at different transverse fields.
 *
 * sga_get_time_links writes B into links [G] (int64, host or device).  Read only: no engine state moves.  Enqueued on the
 * engine's stream behind earlier sweeps; a device buffer returns at once, a host buffer after the copy has landed.
 *   SGA_ERR_INVALID, in this order: engine NULL, "links is NULL", no couplings, no replicas, n_slices < 2, n_slices not
 *   dividing R_local, replica0 not a multiple of n_slices.  Any P >= 2 is served, odd ones included, with no upper bound.
 *   SGA_ERR_UNSUPPORTED: sga_set_tsp, sga_set_groups / sga_set_groups_csr, batches (ragged, shared and stacked).  Everything
 *   else is served -- dense rows in any storage, CSR rows of any class, whatever the rule: no coupling is read.
 *
 * sga_exchange_transverse runs ONE nearest-neighbour exchange round along the group index.  For every lower group a with
 * a % 2 == parity and b = a + 1 < G, in fp64, every operation a single one:
 *   beta_g = 1.0 / T[gP]                       (the temperature of the group's slice 0; equal T within a group is the
 *                                               caller's responsibility, as for the sweeps)
 *   E_g = energy[gP+0] + ... + energy[gP+P-1]  (the tracked energies, left to right)
 *   t1  = (beta_a - beta_b) * (E_a - E_b)
 *   c   = beta_a * (double)k_a - beta_b * (double)k_b
 *   t2  = (2.0 * c) * (double)(B_a - B_b)
 *   x   = t1 + t2;   prob = !(x < 0.0) ? 1.0 : exp(x)   (the deterministic exp of the accept rules)
 *   u   = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53, (w0, w1, ., .) = Philox4x32-10(counter (0, round, a, 8), key = seed)
 *   the groups swap iff u < prob
 * -- the ratio w(a at b's parameters) w(b at a's) / (w(a) w(b)) of the weights exp(-beta H_eff), H_eff = E - k (n P - 2 B).
 * Domain word 8 = sweep | 2 << 2 is no other draw's.  The counter holds the group index: the call needs every group on
 * this rank.  A pair where either T is not positive and finite is left alone.  `round` is the caller's: no counter of the
 * engine moves.
 *   On a swap slice p of a and slice p of b trade their spin rows (all sstride bytes) and their tracked energies (the
 * bits).  Where the cached local fields are valid they trade their resident field rows too, and the fields STAY VALID (F
 * depends on neither k nor T): sga_sweep_transverse_dense, this call, sga_sweep_transverse_dense run without seeding in
 * between.  Where the fields are not valid nothing is done to them; under SGA_FIELD_CACHE_AUTO, where the mark stands for
 * some replicas only, they are marked for re-seeding instead.  Then every slice's best follows where its energy is lower
 * (the step at a sweep's end).  Accept counters, temperatures, slot map, exchange statistics, sweep and round counters and
 * Wolff cursors do not move.
 *   accepted [G] (int32: 1 for both groups of a swapped pair, else 0) and links [G] (int64: B BEFORE the exchange) are host
 * or device buffers or NULL.  G = 1, or a parity that leaves no pair, is a no-op with the outputs still filled.
 *   SGA_ERR_INVALID, first and with nothing enqueued or changed: the ladder above with "k_perp is NULL" and "k_perp holds a
 *   NaN or an infinite value" over the G values, then "parity must be 0 or 1", then "exchanges between groups need every
 *   group on this rank (R_local == R_global)"; k_perp on the device.  SGA_ERR_UNSUPPORTED: the kinds above.
 *   Four launches on the engine's stream with no host round trip between them (the counts, the decision, the swap, the
 *   bests); both calls show in sga_get_last_kernel (time_links_kernel, trotter_exchange_kernel). */
int sga_get_time_links(sga_engine *e, int n_slices, int64_t *links /* host or device [R_local / n_slices] */);
int sga_exchange_transverse(sga_engine *e, int n_slices, const float *k_perp /* host [R_local / n_slices] */, int parity,
                            uint32_t round, int32_t *accepted /* host or device [R_local / n_slices], or NULL */,
                            int64_t *links /* host or device [R_local / n_slices], or NULL */);

/* Stateless operator form of CUDAKernelManager.parallel_tempering_exchange_optimized
 * (annealing/cuda_kernels.py:326-369, fallback :415-443): sequential adjacent pairs, fp32,
 * p = exp((1/T[i+1] - 1/T[i]) * (E[i] - E[i+1])), accepted pairs swap spin rows and energies
 * in place.  spins fp32 [R][n], energies fp32 [R], temps fp32 [R]; u fp32 [R-1] or NULL
 * (Philox, domain 1).  Device or host pointers. */
int sga_op_pt_exchange(int device, float *spins, float *energies, const float *temps,
                       const float *u, uint64_t seed, uint32_t round, int R, int n,
                       int *n_accepted);

/* ---- state access --------------------------------------------------------------------- */
int sga_get_energies(sga_engine *e, double *out /* [R_local] */);
/* Stream-ordered form for a DEVICE destination: the copy is enqueued on the engine's stream and the
 * call returns at once -- for consumers ordered behind that stream (sga_set_stream with the caller's
 * stream: an RCCL all-gather of the energies followed by sga_exchange needs no host synchronisation). */
int sga_get_energies_async(sga_engine *e, double *out_device /* [R_local] */);
int sga_get_temperatures(sga_engine *e, double *out /* [R_local] */);

/* ---- replica observables (version >= 2300; csrc/observables.hip) -------------------------------------------------
 * How the replicas relate to each other, computed where the spins are: one exact integer product Q = A B^T, A the local
 * replicas' int8 spins [R_local][n] and B a set of int8 configurations [C][n], on the int8 matrix cores (both operands
 * read straight from their row-major rows, the K range split over workgroups, partial sums joined by int32 atomics:
 * exact in any order, bit for bit the integer product).  B = A: the overlap matrix n q_ab; B = the best configurations:
 * distances between solutions, d = (n - Q) / 2; B = rows of the caller's: overlaps against an outside state (a planted
 * solution, another rank's spins); one row of ones: the magnetisations.
 *   Pointers: out and cfg may be host or device pointers, as everywhere in this header.  cfg holds int8 values,
 *   normally +-1; a 0 leaves a site out; nothing is checked, the result is the plain dot product.
 *   Stream order: the work is enqueued on the engine's stream behind whatever sweep was enqueued before it.  A host out:
 *   the call returns after the copy has landed; a device out: it returns at once, as sga_get_energies_async does.
 *   Sites are 0 ... n - 1 of the spin rows; what a row holds past n never enters a sum.
 *   Ragged batches (sga_set_csr_batch): rows are zero past n_m, so a magnetisation is over the model's own n_m sites and
 *   a pair of replicas inside a model gets its model's overlap.  A pair ACROSS models gets the dot over the shorter
 *   model's sites: a number without a meaning, computed and not refused.  cfg rows are [n_max].
 *   Every kind of problem is served (the spins in HBM are int8 rows for all of them): one dense model, stacked and
 *   shared batches, CSR with int8 or bit spins in LDS, ragged batches, sga_set_tsp, sga_set_groups with or without a
 *   remainder.  Sharded engines answer for their local replicas; overlaps across ranks are an all-gather of the spins
 *   followed by sga_get_overlaps_with.  Range: n <= ~1.3 10^6 spins, so |Q| < 2^31 for every int8 cfg.
 *   SGA_ERR_INVALID, before anything is enqueued: a NULL engine or out; no problem or no replicas; which outside
 *   {0, 1}; count < 0, or cfg NULL with count > 0 (count = 0 is a no-op); ld < n; ldq < R_local (sga_get_overlaps) or
 *   ldq < count (sga_get_overlaps_with).
 *   Read only: no replica state, cached field, counter, best, window plan or sga_get_last_kernel text changes, and the
 *   engine keeps no state for these calls (scratch: the staging slots of the single-site operators).  A run with these
 *   calls interleaved walks the same chain as one without them.
 * (Reference: core/spin_dynamics.py:90-92, magnetization_history = sum_i s_i per sweep; it has no overlaps.) */
#define SGA_SPINS_CURRENT 0   /* the replicas' spins, as sga_get_spins returns them   */
#define SGA_SPINS_BEST    1   /* the best configurations, as sga_get_best returns them */
/* out[r] = sum_i s_r[i], local replica r (ragged batches: over the model's own n_m sites) */
int sga_get_magnetizations(sga_engine *e, int which, int32_t *out /* [R_local] */);
/* out[a * ldq + b] = sum_i A_a[i] B_b[i] over all local replicas a, b; A = which_a, B = which_b */
int sga_get_overlaps(sga_engine *e, int which_a, int which_b, int32_t *out, int64_t ldq /* >= R_local */);
/* out[a * ldq + c] = sum_i A_a[i] cfg[c * ld + i] : the local replicas against caller-supplied configurations */
int sga_get_overlaps_with(sga_engine *e, int which, const int8_t *cfg, int64_t ld /* >= n */, int count,
                          int32_t *out, int64_t ldq /* >= count */);

int sga_get_spins(sga_engine *e, int r, int8_t *out /* [n]; r<0: all, [R_local][n] */);
int sga_set_spins(sga_engine *e, int r, const int8_t *s /* recomputes that energy */);
/* r >= 0: best (energy, spins) seen by local replica r at sweep ends; r < 0: the best over
 * all local replicas; *r_out (optional) receives its local index. */
int sga_get_best(sga_engine *e, int r, double *energy, int8_t *spins /* [n] or NULL */,
                 int *r_out);
/* Forget the bests: best = current state (ParallelTempering checks only on record sweeps). */
int sga_reset_best(sga_engine *e);
int sga_get_stats(sga_engine *e, int64_t *accepted /* [R_local] */,
                  int64_t *attempted /* [R_local] */);
int sga_get_slot_map(sga_engine *e, int32_t *slot_to_rep /* [R_global] */);
int sga_get_exchange_stats(sga_engine *e, int64_t *attempts /* [R_global] */,
                           int64_t *accepts /* [R_global] */);
/* What a tempering host loop reads at an event -- energies [R_local], acceptance counters
 * [R_local], the ladder permutation [R_global] (any may be NULL) -- with ONE synchronisation
 * (ParallelTempering._record_statistics / acceptance bookkeeping, parallel_tempering.py:295-301). */
int sga_snapshot(sga_engine *e, double *energies, int64_t *accepted, int32_t *slot_to_rep);
/* Philox key of all later draws (sweeps, exchanges); the counters are unchanged. */
int sga_set_seed(sga_engine *e, uint64_t seed);
int sga_get_sweep_counter(sga_engine *e, uint32_t *sweeps_done, uint32_t *exchange_rounds);
int sga_set_sweep_counter(sga_engine *e, uint32_t sweeps_done, uint32_t exchange_rounds);

/* ---- checkpoint / resume ---------------------------------------------------------------- */
/* Everything that makes a run continue bit-exactly -- spins, tracked and best energies, best
 * configurations, temperatures, ladder permutation and statistics, acceptance counters, seed
 * and stream counters -- as one host blob.  sga_export_state with buf == NULL only reports the
 * size.  Import needs an engine holding the same problem with replicas (and ladder, if one was
 * exported) initialised to the same counts.  (The reference can only save final results:
 * AnnealingResult.save, annealing/result.py:147-165.) */
int sga_export_state(sga_engine *e, void *buf, uint64_t capacity, uint64_t *needed);
int sga_import_state(sga_engine *e, const void *buf, uint64_t size);

/* ---- measurement ---------------------------------------------------------------------- */
/* With timing enabled every sweep-kernel launch is bracketed by HIP events on the launch
 * stream; sga_get_kernel_time returns the launches and their summed duration since the
 * last reset (synchronises). */
int sga_enable_timing(sga_engine *e, int on);
int sga_get_kernel_time(sga_engine *e, int64_t *n_launches, double *total_ms, int reset);
/* Describes the launch geometry chosen for the current problem (for DESIGN/bench output):
 * writes a NUL-terminated string into buf. */
int sga_describe(sga_engine *e, char *buf, int buflen);
/* 64-bit checksum of the problem as the sweep kernels read it (packed couplings / entry layout /
 * distance tables, and h).  Ranks of a sharded run compare it after set-up: every rank must hold the
 * same couplings (the reference replicates the model per device, annealing/multi_gpu.py:110-132). */
int sga_problem_checksum(sga_engine *e, uint64_t *out);
/* Launch geometry of the dense sweep kernels (sga_set_tuning / sga_autotune / heuristic). */
int sga_get_geometry(sga_engine *e, int *waves_per_replica, int *chunks_per_wave);
/* Measurement aid: the kernel instantiation (template arguments, waves per replica) that the calling
 * thread's last sga_sweep launched -- what a rocprofv3 trace of the same command must show. */
int sga_last_kernel(char *buf, int buflen);
/* Measurement aid: GB/s of a plain streaming read (every workgroup its own segment, eight non-temporal 16-byte loads per lane in flight) of a fresh `bytes`-byte
 * device buffer, `reps` passes -- the practical bandwidth of this device beside its spec figure. */
int sga_probe_read_bandwidth(int device, int64_t bytes, int reps, double *gb_per_s);
/* Storage of CSR entries in the one-replica-per-workgroup bit-spin sweep forms (long rows; call before
 * sga_init_replicas).  AUTO: integer-valued problems with |J| <= 127 and n < 2^24 keep a second layout
 * with one dword per entry (24-bit column | 8-bit value) -- half the bytes per row, identical chains;
 * F32: always the (column int32, value fp32) entries; PACKED: fail (SGA_ERR_UNSUPPORTED, at
 * sga_init_replicas) when the packed layout cannot be used.  The choice is latched by
 * sga_init_replicas: a call made while replicas exist takes effect at the next sga_init_replicas
 * (sga_describe reports what the current replicas run).  (No reference counterpart: the
 * reference stores torch COO / dense fp32, core/ising_model.py:56-63.) */
#define SGA_CSR_STORAGE_AUTO 0
#define SGA_CSR_STORAGE_F32 1
#define SGA_CSR_STORAGE_PACKED 2
int sga_set_csr_storage(sga_engine *e, int storage);
/* How sga_sweep evaluates a proposal.  OFF (default): the reference's way -- the local field of the
 * proposed site is formed from its coupling row (IsingModel.get_local_field, core/ising_model.py:176-185):
 * one row read per proposal.  ON / AUTO: the local fields of every replica stay resident in LDS and a row is
 * read only when a proposal is ACCEPTED, to update them -- the reference's incremental mode,
 * core/energy_computer.py:166-173,262-265.  Same sites, uniforms and accept rule on exact integers: the chain
 * equals OFF's bit for bit.  Served:
 *   dense couplings (sga_set_dense, one model): J integer valued and symmetric with a zero diagonal, h in
 *     multiples of 1/2, max_i(sum_j |J_ij| + |h_i|) < 2^24 (2^23 with half-integer h), n <= ~75 000 (int16
 *     fields; ~37 000 with int32); fields seeded by one pass over J on the matrix cores; any rule but
 *     SGA_RULE_WOLFF, every site mode and arithmetic;
 *   dense batches (sga_set_dense_batch, M models of one size; version >= 900): the same conditions over ALL stacked
 *     rows -- scale, field width and accept table are batch-wide, which keeps every model's fields exact and its
 *     chain the one-model chain; fields seeded by one launch of exact integer sums, eight replicas per pass over
 *     a model's rows; "several accepts per round" needs each MODEL's matrix below 4 GiB, not the stack's;
 *     sga_explain_route / sga_describe name the batch ("models=M").  The fixed-point form over batches stays
 *     refused unless option "batch_fixed_point" = 1 is set beside "clf_fixed_point" = 1 (version >= 1400): then the
 *     conditions of the one-model fixed-point form over all stacked rows, one k and one width (int32 | int64) for the
 *     batch, fields seeded by one launch of exact fp64 sums (eight replicas of one model per pass), any single-site
 *     rule, site mode and arithmetic, one accept per round; AUTO routes each replica by its own acceptance against
 *     the one-model dense fixed-point break-even (not measured for batches);
 *   ragged CSR batches (sga_set_csr_batch; version >= 1100) under option "ragged_field_cache" = 1: the CSR
 *     conditions below in every model, production sweeps, one launch under AUTO decided by the hottest replica.
 *     With the option at 0 (default) ON is refused (SGA_ERR_UNSUPPORTED) and AUTO streams.  With option
 *     "clf_fixed_point" = 1 as well (version >= 1300) a batch that fails those conditions is served by the fixed-point
 *     form -- one k and one field width (int32 | int64) for the batch, any fp32 h, any single-site rule and
 *     arithmetic on Philox sites; AUTO by the hottest replica against the one-model fixed-point break-even (~6 % int64,
 *     ~3.4 % int32; not measured for ragged batches);
 *   CSR couplings (sga_set_csr, or a sparse matrix sga_set_dense kept as CSR): J integer valued and symmetric
 *     in strictly sorted rows (no duplicate entries), zero diagonal, h in multiples of 1/2,
 *     max_i sum_j |J_ij| < 2^15 (only the dynamic part J s of a field is kept, as int16; h is read beside it),
 *     rows of <= 2048 entries, n <= ~72 000; production sweeps (SGA_SITE_RANDOM, SGA_ARITH_F64, Metropolis, no
 *     per-update records) -- other arguments take OFF's kernels for that call, the same chain.
 * ON: sga_sweep fails with SGA_ERR_UNSUPPORTED where the problem does not qualify.  AUTO: falls back to OFF's
 * kernels there -- and while replicas are hot: it starts on OFF's kernels (on the cached fields where the break-even
 * below is above ~0.3: nothing is known yet, and there the row kernels lose more on a cold ladder than the cached
 * fields on a hot one), reads the per-replica acceptance
 * counters back every 4 ... 16 sweeps (when a sga_sweep call starts; a long production call is walked in pieces of 16 sweeps for that) and
 * then routes EACH replica of a dense problem by its own acceptance
 * (break-even = what an update costs its chain on OFF's kernel over what an accept costs it here: 0.25 on
 * bit-planes, 0.39 on int8 rows at n = 10^4, never on fp32 rows): a ladder with a hot end runs as two concurrent
 * launches over disjoint replica lists (option "replica_routing" = 0, and CSR problems: one launch, decided by the
 * hottest replica).  Cost model: an accepted proposal costs ~1.1 - 1.7 us of its replica's serial chain, a
 * rejected one next to nothing -- 100-450 x OFF in the glassy regime annealing ends in. */
#define SGA_FIELD_CACHE_OFF 0
#define SGA_FIELD_CACHE_ON 1
#define SGA_FIELD_CACHE_AUTO 2
int sga_set_field_cache(sga_engine *e, int mode);

/* Sequential windows (version >= 2100; csrc/sweep_dense_seq.hip): SGA_SITE_SEQUENTIAL sweeps of many replicas with ONE
 * read of each coupling row per sweep.
 * W = 0 (default): off, nothing changes.  W = 256 | 512 | 1024: on, wherever the form applies.
 * Any other value: SGA_ERR_INVALID.  Read at every sga_sweep; kept across sga_set_* calls, as sga_set_field_cache is.
 * In typewriter order every replica proposes the same W sites inside a window of W consecutive updates: the
 * window-start row sums of all replicas are one (W x n) . (n x R) product on the matrix cores (int8 cores for int8
 * rows and for fp32 rows with |2^k J_ij| <= 127, else the fp32 cores), and one wave per replica then walks the window's
 * chain, correcting the fields for the window's earlier accepts from the accepted sites' rows.  The chain, energies,
 * counters and bests are the row-per-proposal kernel's, bit for bit.
 * The form runs where all of these hold, otherwise that call runs today's kernel: site_mode == SGA_SITE_SEQUENTIAL
 * (uniforms from Philox or replay_u), no accept_trace / dE_trace (energy_trace is served), Metropolis in either
 * arithmetic or Glauber / heat bath (never Wolff), field cache OFF, J symmetric with a zero diagonal, option
 * "force_general" = 0, one dense matrix (one model or sga_set_dense_shared; not a stacked batch, CSR, TSP or groups),
 * R n < 2^31, and a problem class in which the product is exact: J and h integer valued with every partial sum below
 * 2^24 (the accept table's class), or -- under option "row_shared_grid" = 1 -- J on a binary grid 2^-k with scaled sums
 * below 2^24 and any finite h (integer J beside a half-integer or real h is k = 0).  Option "row_shared" does not gate
 * it.  sga_describe shows " sweep=seq-windows(W=...)" while the setting is on and the problem qualifies,
 * sga_get_last_kernel names sweep_dense_seq<...>; sga_explain_route keeps its random-site answer (a query carries the
 * site mode no more than the rule).  The setting is not part of sga_export_state. */
int sga_set_sequential_windows(sga_engine *e, int W);
int sga_get_sequential_windows(sga_engine *e, int *W);
/* Replica groups (version >= 2400; csrc/sweep_dense_rs.hip): replicas are independent inside a sweep, so the row-shared
 * sweep over the tile plan (its fields in tiles of sites, option "row_shared_fields") cuts them into contiguous groups
 * and runs each group's whole sweep -- plan, fields and chain per window, best tracking -- on a stream of its own: one
 * group's chain runs beside another's fields.  Every group is forked from the engine's stream when a launch starts and
 * joined into it before the launch returns, so whatever follows on that stream sees all replicas done.  No result
 * changes: a replica's chain is the one-group chain, bit for bit.
 * g = 0 (default): the count is the rule's -- two groups where each gets at least 256 replicas, else one (four measured
 * slower than two and are only ever forced).
 * g = 1 | 2 | 4: that count wherever the form admits groups (fewer where R gives fewer ranges: every inner boundary is a
 * multiple of 32).  Any other value: SGA_ERR_INVALID.  Read at every sga_sweep; kept across sga_set_* calls; not part of
 * sga_export_state.  One group runs wherever the tile plan does not (the per-site fields kernel, the sequential windows,
 * every other sweep form) and while an energy trace is asked for.  sga_describe and sga_get_last_kernel end in
 * " groups=G" where more than one group runs -- at one they are what they were -- and sga_describe in " groups=no(why)"
 * where g > 1 was asked for and one runs. */
int sga_set_replica_groups(sga_engine *e, int g);
int sga_get_replica_groups(sga_engine *e, int *g);
/* Form-selection options of ONE engine -- the A/B switches of the measurements and what the parity tests use to
 * force a kernel form -- by name.  None changes a result: every form walks the same chain.  The
 * environment is read once, in sga_create, for the defaults (variable in brackets); afterwards only these calls
 * count, so two engines of one process can run different forms.  SGA_ERR_INVALID: unknown key, value out of range.
 * When a value takes effect: [set] at the next sga_set_dense / sga_set_csr, [init] at the next sga_init_replicas,
 * [sweep] at the next sga_sweep / sga_recompute_energies.  A [set] option changed while couplings are set, or an
 * [init] option changed while replicas exist, cannot act on them any more: sga_sweep then refuses (SGA_ERR_INVALID,
 * naming the key) until the couplings / replicas are set up again -- it never silently runs the form the old value chose.
 *   "look_ahead"            0 | 1 (default)   dense integer problems: several updates reduced together  [sweep; SGA_NO_LOOK_AHEAD]
 *   "force_general"         0 (default) | 1   general kernel builds even for production arguments       [sweep; SGA_FORCE_GENERAL]
 *   "clf_waves"             0 = measured table (default), 1 ... 16 (capped at 8): waves per replica of the windowed cached-field
 *                           sweep (a value selects that form)                                       [sweep; SGA_CLF_WAVES]
 *   "clf_tail_waves"        0 | 1 (default)   cached-field sweep over dense couplings (ON and AUTO): the per-replica
 *                           acceptance is looked at every 4 ... 16 sweeps (when a sga_sweep call or one of its 16-sweep pieces starts); once the mean is below 0.28 of the
 *                           hottest replica's -- the launch is that replica's chain, the chip idles behind it -- every
 *                           replica runs at eight waves.  Same chain                          [sweep; SGA_NO_CLF_TAIL_WAVES]
 *   "clf_batched"           2 (default) | 1 | 0   cached-field sweep under production arguments commits SEVERAL accepts per
 *                           round: all decisions of a window guessed at once, the guess checked against the couplings
 *                           between the accepting sites, the rows applied two at a time (csrc/sweep_clfb_impl.h).  Same
 *                           chain.  2 = while the hottest replica accepts more than ~1 % of its proposals (where the
 *                           form is ahead), 1 = always, 0 = never                               [sweep; SGA_CLF_BATCHED]
 *   "clf_fixed_point"       0 (default) | 1   cached-field sweep over CSR couplings for real-valued J and wide
 *                           integer fields: D_i = 2^k sum_j J_ij s_j kept EXACTLY as int32 | int64 in LDS (k from the
 *                           set-time scan of J's binary exponents; acc class f32 / f64-exact, symmetric J in strictly
 *                           sorted rows, zero diagonal, any fp32 h), dot = fp32(2^-k D_i) -- the row kernels' value --
 *                           and the same accept rule: the same chain, any single-site rule, site mode and arithmetic.
 *                           Problems the int16 form serves keep it.  Refused: f64-canonical J, the implicit TSP form,
 *                           fields past LDS.  Ragged batches (sga_set_csr_batch): refused unless option
 *                           "ragged_field_cache" = 1 is set too -- then one k and one width for the batch, see there.
 *                           DENSE couplings (sga_set_dense, one model) that the integer cached-field form does not take
 *                           -- real-valued J, or integer J beside an h that is no multiple of 1/2 --: the same D_i in
 *                           LDS (csrc/sweep_clf_fx.hip), conditions as above (acc class f32 / f64-exact, symmetric J,
 *                           zero diagonal, any fp32 h; k = 0 for integer J), int32 while 2^k max_i (sum_j |J_ij| +
 *                           |h_i|) < 2^31, else int64.  fp32 rows, int8 rows (integer J, k = 0) and bit-plane storage
 *                           (its int8 rows are read on accept) are served.  Refused, each with its reason
 *                           (sga_describe / the error of SGA_FIELD_CACHE_ON): f64-canonical J, asymmetric J, a non-zero
 *                           diagonal, dense batches, fields wider than int64, fields and spins of a replica past LDS
 *                           (160 KiB: n <= ~39 000 int32, ~20 000 int64).  Problems the integer form serves keep it;
 *                           option "clf_batched" does not apply (one accept per round)                  [set]
 *   "replica_routing"       0 | 1 (default)   SGA_FIELD_CACHE_AUTO routes each replica by its own acceptance (two
 *                           concurrent launches) instead of the whole launch by the hottest replica    [sweep; SGA_NO_REPLICA_ROUTING]
 *   "batched_energy"        0 = one pass over the couplings per replica, 1 (default) = all replicas in one pass where
 *                           that carries the same bits (not for real-valued couplings that need the canonical
 *                           summation order; CSR: only where X is exact in fp64), 2 = always           [sweep; SGA_NO_MFMA_ENERGY]
 *   "fields_scratch_mb"     256 (default): cap in MiB of the scratch of the all-replica field / energy pass over dense
 *                           couplings; larger replica sets go through in tiles of 128-replica blocks    [sweep; SGA_FIELDS_SCRATCH_MB]
 *   "csr_updates_per_step"  -1 = by the longest row (default), 0 = one update at a time, 1 | 2 = pair look-ahead,
 *                           4 | 8 = that many updates per step (rows <= 256 entries)                    [init, sweep; SGA_CSR_PAIR_AHEAD]
 *   "tsp_updates_per_step"  -1 = by the number of cities (default), 0 | 1 = one, 2 | 4 | 8              [sweep; SGA_TSP_PARALLEL]
 *   "sparse_route"          0 | 1 (default)   sga_set_dense keeps a sparse integer matrix as CSR        [set; SGA_NO_SPARSE_ROUTE]
 *   "csr_slots"             0 | 1 (default)   long-row CSR problems padded to 64-entry slots at set time [set; SGA_NO_CSR_SLOTS]
 *   "half_integer_table"    0 | 1 (default)   accept table for integer J with half-integer h            [set; SGA_NO_HALF_TABLE]
 *   "force_csr_acc"         0 (default) ... 3: at least this CSR_ACC class (1 f32, 2 f64, 3 f64 canonical) [set; SGA_FORCE_CSR_ACC]
 *   "force_dense_canonical" 0 (default) | 1   canonical fp64 order for every fp64-accumulated dense problem [set; SGA_FORCE_DENSE_CANON]
 *   "zero_slot_every"       0 = 2^21 (default), k: an all-zero slot inside the slotted layout after every k slots [set; SGA_ZERO_SLOT_EVERY]
 *   "csr_bits"              0 | 1 (default)   bit spins where they keep more replicas LDS resident      [init; SGA_NO_CSR_BITS]
 *   "force_csr_bits"        0 (default) | 1   CSR sweeps with bit spins whatever the size               [init; SGA_FORCE_CSR_BIG]
 *   "row_shared"            0 | 1 | 2 (default)   dense integer problems (one model, or the models of sga_set_dense_shared; J and h integer with exact fp32 sums,
 *                           J symmetric with a zero diagonal, |J| <= 255), production sweeps with the field cache off:
 *                           "row-shared windows" (csrc/sweep_dense_rs.hip) -- each sweep cut into windows of W updates per
 *                           replica, each proposed row read ONCE per window and dotted with the window-start spins of every
 *                           replica that proposes it, the chain then walked per replica with exact corrections for the
 *                           window's earlier accepts.  Same chain.  The rule: SGA_RULE_METROPOLIS decides with the accept
 *                           table; SGA_RULE_GLAUBER and SGA_RULE_HEAT_BATH (version >= 2000) decide with the row kernels'
 *                           general fp64 rule on the same exact fields -- sga_describe and sga_get_last_kernel then say
 *                           "rule=glauber" / "rule=heat-bath" --; SGA_RULE_WOLFF is never served.  0 = never, 1 = wherever
 *                           it applies (W: option "row_shared_window"), 2 = where sga_autotune measured it ahead of every
 *                           geometry by more than 1 %, under the rule the engine had when it measured: after
 *                           sga_set_update_rule to another rule the row-per-proposal kernel runs until sga_autotune is
 *                           called again.  Measured at n = 10^4, 1024 replicas (profiles/row_shared_rules.json): +-1 J,
 *                           integer h 21.8 -> 1.22 ms per sweep under Glauber, 22.1 -> 1.21 under heat bath; J = +-1/4
 *                           with "row_shared_grid" 57.8 -> 1.90 and 57.9 -> 1.86                    [sweep; SGA_ROW_SHARED]
 *   "row_shared_grid"       0 (default) | 1   (version >= 1800) opens the row-shared windows to dense problems the integer form
 *                           does not take: every J_ij a multiple of 2^-k (k <= 30, integer J: k = 0) with 2^k |J_ij| <= 255
 *                           and 2^k max_i (sum_j |J_ij| + |h_i|) < 2^24, J symmetric with a zero diagonal and not all zero, h
 *                           ANY finite fp32 (quarter-valued QUBO encodings, integer J beside a real-valued h).  The planes hold
 *                           2^k J, the chain decides with the row kernels' general rule: same chain.  Acts where "row_shared"
 *                           does (field cache off; 1 forces the form, 2 lets sga_autotune time it); a shared-coupling batch
 *                           qualifies as a whole (k, planes and the bound over the batch).  0: nothing changes
 *                                                                                          [sweep; SGA_ROW_SHARED_GRID]
 *   "row_shared_fields"     0 | 1 | 2 (default)   (version >= 1900) the fields kernel of the row-shared windows over resident
 *                           bit-planes: 0 = one workgroup per proposed site; 1 | 2 = one workgroup per tile of S consecutive
 *                           sites, the tile's plane rows in LDS and its entries grouped by replica, so that a replica's spin
 *                           bits are read once per tile instead of once per proposal; where every off-diagonal |J_ij| (grid
 *                           form: |2^k J_ij|) is 1 the rows are their sign planes alone ("sign-only").  1: wherever the kernel
 *                           can run; 2: where it was measured to win -- sign-only rows, 7936 < n <= 16384 (a replica's spin
 *                           bits of 1 KB or more, within the kernel's registers).  The per-site kernel
 *                           still runs where R exceeds 4096 (the kernel's replica counters), two rows' planes do not fit the
 *                           tile image, or the runtime refuses the LDS: sga_describe says which (rs_tiles=...).  Same chain
 *                                                                                        [sweep; SGA_ROW_SHARED_FIELDS]
 *   "row_shared_tile_sites" 0 (default) = S by the library's rule, else S, 2 ... 4096 (tests, A/B runs)
 *                                                                                    [sweep; SGA_ROW_SHARED_TILE_SITES]
 *   "row_shared_window"     0 (default) | 256 | 512 | 1024 (other values: rounded down): W under "row_shared" = 1 (0: the
 *                           autotuner's, else 1024)                                      [sweep; SGA_ROW_SHARED_WINDOW]
 *   "ragged_field_cache"    0 (default) | 1   ragged CSR batches (sga_set_csr_batch): the int16 cached-field sweep of
 *                           sga_set_csr over the batch (csrc/sweep_clf_csr.hip, ragged build): sga_set_field_cache(ON)
 *                           is accepted, sga_set_csr_batch scans every model for the form's conditions, ON / AUTO act
 *                           as on a one-model CSR engine.  0: ON is refused, AUTO streams.  Same chain.  Together with
 *                           option "clf_fixed_point" = 1 (version >= 1300): a batch the int16 form does not take runs
 *                           the fixed-point form over the batch (int32 | int64 fields at one batch-wide k)  [set]
 *   "batch_fixed_point"     0 (default) | 1   many-model dense batches (sga_set_dense_batch) under option "clf_fixed_point"
 *                           = 1, both set before the couplings: a batch the integer cached-field form does not take runs
 *                           the dense fixed-point form (csrc/sweep_clf_fx.hip, batch build) -- one k (the finest grid any
 *                           model's J needs) and one field width (int32 | int64) for the batch, each replica on its own
 *                           model's rows and h, every model on its one-model chain.  0, or "clf_fixed_point" = 0: as
 *                           before -- ON over such a batch is refused ("not built for dense batches"), AUTO runs the
 *                           row kernels.  Bit-plane storage, row-shared windows and "clf_batched" do not apply to
 *                           batches in fixed point                                         [set; SGA_BATCH_FIXED_POINT]
 * sga_option_name enumerates the keys (index 0, 1, ... until SGA_ERR_INVALID).
 * (No reference counterpart: the reference has one code path, core/spin_dynamics.py:61-152.) */
int sga_set_option(sga_engine *e, const char *key, int64_t value);
int sga_get_option(sga_engine *e, const char *key, int64_t *value);
int sga_option_name(int index, char *buf, int buflen);
/* Tuning override (0 = heuristic): waves per replica and sweeps per launch. */
int sga_set_tuning(sga_engine *e, int waves_per_replica, int sweeps_per_launch);
/* Measured choice of the launch geometry / sweep form: times the sweep kernel for every feasible candidate on the
 * current replicas (a few sweeps each) and keeps the fastest -- dense problems: waves per replica; CSR problems
 * (round 4): waves per replica x several updates per step or one, i.e. every form sga_init_replicas chooses between
 * by thresholds (the state travels through the geometry-independent blob of sga_export_state).  The chain does not
 * depend on the form and the replicas' state, best states, counters and kernel-timing statistics are restored, so
 * results are unaffected.  Candidates within 1 % of the fastest are a tie, which goes to the fewest waves / the simpler
 * form (a fixed preference order: other boxes and later profiles see the same pick).  The pick stays as
 * sga_set_tuning / option "csr_updates_per_step" would have set it (readable through sga_get_geometry /
 * sga_get_option) for as long as THIS problem is held, another sga_init_replicas included.  It ends with the problem
 * it was measured on: the next sga_set_* call returns to the caller's own values -- what the caller last passed to
 * sga_set_tuning and sga_set_option("csr_updates_per_step"), or the defaults -- sga_get_option reads the caller's value
 * again and the table of sga_get_autotune_table is empty.  Dense problems under option "row_shared" = 2 also time the row-shared windows at W = 256, 512 and
 * 1024 on the winning geometry, each after 16 untimed sweeps at that window from the saved state (the form's time depends on
 * the acceptance, which falls steeply in the first sweeps of a run), over at least 16 timed sweeps (table entries "row-shared:W<W>") and keep the fastest where it beats the fastest
 * geometry by more than 1 %; *best_ms_per_sweep is the fastest GEOMETRY's figure either way.  The trials sweep under the engine's update
 * rule (Metropolis, Glauber or heat bath; version >= 2000) and the window kept holds for that rule only: after sga_set_update_rule to another rule the
 * row-per-proposal kernel runs until sga_autotune is called again.  No-op for sga_set_tsp problems.
 * (No reference counterpart: the reference has no launch geometry.) */
int sga_autotune(sga_engine *e, double *best_ms_per_sweep);
/* What the last sga_autotune of this engine measured: "candidate=ms per sweep;..." (dense: "<waves>x<chunks per wave>",
 * the first entry "heuristic:..." being the untuned choice; CSR: the kernel instantiation).  Empty before. */
int sga_get_autotune_table(sga_engine *e, char *buf, int buflen);

/* ---- form selection, inspectable without a GPU ---------------------------------------------------------------
 * WHICH kernel form sweeps a problem (never what it computes) is a pure function of the problem's traits -- what the
 * set-time scans found -- the replica count, the tuning and the options: csrc/sga_route.cpp, a translation unit
 * without a device call.  The engine fills a sga_route_query from its own state and asks that function; tests fill
 * one by hand and pin the answer (tests/test_host_logic.py: the five BASELINE configs and the fuzz shapes).
 * (No reference counterpart: the reference has one code path, core/spin_dynamics.py:61-152.) */
#define SGA_ROUTE_DENSE 0
#define SGA_ROUTE_CSR 1
#define SGA_ROUTE_TSP 2
#define SGA_ROUTE_GROUPS 3
#define SGA_ROUTE_MAX_OPTS 32
typedef struct sga_route_query {
    int32_t kind;         /* SGA_ROUTE_DENSE | SGA_ROUTE_CSR | SGA_ROUTE_TSP (sga_set_tsp) | SGA_ROUTE_GROUPS (sga_set_groups) */
    int32_t n;            /* spins */
    int32_t n_models;     /* dense batches (sga_set_dense_batch), ragged CSR batches (sga_set_csr_batch), else 1 */
    int32_t R_local;      /* replicas on this engine (0: none yet) */
    int32_t cus;          /* compute units of the device (MI355X: 256) */
    int32_t tune_waves;   /* sga_set_tuning waves_per_replica (0 = heuristic) */
    int32_t field_cache;  /* SGA_FIELD_CACHE_* */
    /* what the set-time scans found */
    int32_t storage;      /* dense: SGA_J_F32 | SGA_J_I8 | SGA_J_T2 as resolved; CSR: SGA_CSR_STORAGE_* as requested */
    int32_t acc;          /* dense: 0 fp32 (exact) | 1 fp64, any order | 2 fp64 canonical order;
                             CSR: 0 fp32 + accept table | 1 fp32 | 2 fp64 | 3 fp64 canonical */
    int32_t table_m;      /* entries of the accept table (integer problems), 0 = none */
    int32_t table_scale;  /* 2: half-integer fields, table at twice the resolution */
    int32_t clf_ok;       /* the problem qualifies for the cached-local-field sweep (integer, symmetric, ...) */
    int32_t clf_bits;     /* dense: 16 | 32-bit resident fields */
    int32_t clf_scale;    /* dense: 2 = half-integer fields */
    int32_t from_dense;   /* CSR taken from a sparse matrix handed over dense */
    /* CSR structure */
    int64_t nnz;          /* entries (TSP: 4 (cities - 1) n) */
    int64_t max_row_len;  /* entries of the longest row */
    int64_t layout_entries; /* entries of the layout the kernels read (padding included) */
    int32_t slotted;      /* rows padded to whole 64-entry slots */
    int32_t rowptr32;     /* the layout has < 2^31 entries: 32-bit extents exist */
    int32_t packed_ok;    /* every entry fits the packed form (integer |J| <= 127, n < 2^24) */
    int32_t n_cities;     /* TSP */
    /* as laid out (0 = derive from the rest) */
    int32_t sstride;      /* spin stride of the replicas */
    int32_t shared_j;     /* batches (n_models > 1): 1 = one coupling matrix for every model -- SGA_ROUTE_DENSE: sga_set_dense_shared (version >= 1600); SGA_ROUTE_CSR: sga_set_csr_shared (version >= 1700; 0 = a ragged batch) */
    int64_t ldj;          /* dense: row stride of the packed couplings in elements */
    int64_t opt[SGA_ROUTE_MAX_OPTS]; /* option values, index = sga_option_name order */
    /* sga_set_groups (version >= 1000) */
    int32_t n_groups;     /* groups */
    int32_t group_max;    /* members of the largest group */
    /* sga_set_groups_csr (version >= 1200): the stored remainder, 0 = none */
    int64_t rest_nnz;     /* entries */
    int32_t rest_max_row; /* entries of the longest row */
    int32_t rs_grid;      /* dense (version >= 1800): 0 = the set-time scan gave no grid verdict for the row-shared windows
                             (option "row_shared_grid"), else 1 + k: J on the grid 2^-k */
} sga_route_query;
/* zeroes *q and fills the option defaults (the environment is NOT consulted), cus = 256, n_models = 1 */
int sga_route_query_init(sga_route_query *q);
/* one line naming every decision for q: "dense storage=... waves=... chunks_per_wave=... kernel=..." |
 * "csr form=rows|narrow|narrow-bits|wide-bits|wide-bytes spins=... waves=... updates_per_step=..." | "tsp waves=... passes=..." |
 * "groups n_groups=... sums=int16|int32 waves=... kernel=sweep_groups_kernel|sweep_groups_general_kernel"
 * (with a stored remainder, rest_nnz > 0: " rest_nnz=... rest_max_row=..." behind it)
 * followed by " cached=..." (what sga_set_field_cache would run).  Pure: no device needed.
 * A query does not carry the update rule: the line is the SGA_RULE_METROPOLIS answer (" sweep=row-shared(...)" under
 * option "row_shared" = 1 included); sga_describe and sga_get_last_kernel name the rule an engine sweeps under. */
int sga_explain_route(const sga_route_query *q, char *buf, int buflen);
/* the query the engine itself would pose for its current problem / replicas / options */
int sga_get_route_query(sga_engine *e, sga_route_query *out);
/* The raw words the set-time scans wrote for the problem as it is held (version >= 1500).  No device call: the setter
 * keeps what it read back.  words may be NULL (then only *kind and *count are filled); else capacity >= *count.
 * *kind = SGA_ROUTE_DENSE: 8 words; a dense batch is scanned stacked (every word is over all models' rows): model must be 0.
 *   [0] 1: some J_ij is not an integer in [-127, 127] (0: J fits int8)
 *   [1] 1: some J_ij is outside {-1, 0, +1}
 *   [2] float bits of max_i (sum_j |J_ij| + |h_i|): the fp32 rounding of the fp64 sum
 *   [3] bit 0: some J_ij is not an integer; bit 1: some h_i is not an integer; bit 2: some h_i is not a multiple of 1/2
 *       (bit 3, non-finite input, is never seen here: such a problem is refused)
 *   [4] 1: some model's J is not symmetric or has a non-zero diagonal entry
 *   [5] 1024 + e_hi, [6] 1024 - e_lo: the binary exponents of the highest and the lowest set bit of any non-zero J_ij
 *       (subnormals by their true bits: 3 x 2^-149 has e_hi = -148, e_lo = -149); both 0 when J is all zero
 *   [7] float bits of max |J_ij|
 * *kind = SGA_ROUTE_CSR: 11 words per model (ragged batches: model = 0 .. n_models - 1), the stored entries only:
 *   [0] bad rowptr and [1] bad column (0: either is refused)
 *   [2] the bits of dense word [3]
 *   [3] 1: some row is not strictly ascending by column (unsorted, or a column twice)
 *   [4] 1: a non-zero diagonal entry        [5] 1: J_ij != J_ji for some stored entry (duplicates summed)
 *   [6] float bits of max_i (sum_j |J_ij| + |h_i|)   [7] 1024 + e_hi   [8] 1024 - e_lo   (as dense [5], [6])
 *   [9] float bits of max_i sum_j |J_ij|    [10] entries of the longest row
 * A dense matrix kept as CSR (sga_get_route_query: from_dense) reports the CSR words.
 * sga_set_tsp / sga_set_groups*: SGA_ERR_UNSUPPORTED (scanned on the host, no words kept). */
int sga_get_scan_summary(sga_engine *e, int model, int32_t *kind, int32_t *words, int capacity, int *count);
/* the instantiation this ENGINE's last sweep launch ran (sga_last_kernel: this thread's last launch of any engine) */
int sga_get_last_kernel(sga_engine *e, char *buf, int buflen);

#ifdef __cplusplus
}
#endif
#endif /* SGA_H */
