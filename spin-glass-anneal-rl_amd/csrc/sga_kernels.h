// sga_kernels.h -- kernel argument blocks and host-callable launchers shared between the
// kernel translation units (*.hip) and the C-ABI engine (sga_engine.cpp); the replica measurements and moves beside the
// sweeps stand in sga_replicas.h, simulated quantum annealing in sga_quantum.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sga {

// The instantiation the last sweep launch of this thread ran (measurement: bench.py writes it beside
// the roofline figure, so that a profile can be matched to the timed kernel).
void note_sweep_kernel(const char *fmt, ...);
const char *last_sweep_kernel();

// Raise a kernel's dynamic-LDS limit once per (device, kernel, size), not on every launch.
hipError_t ensure_lds_limit(const void *kernel, size_t lds_bytes);

constexpr int MAX_CPW = 10;       // coupling-row chunks a wave holds per buffer (dense)
constexpr int T2_MAX_CPW = 4;     // same for the bit-plane form (a chunk is two planes = 8 VGPRs)
constexpr int MAX_WAVES = 16;     // waves per replica workgroup
constexpr int CSR_WAVES_PER_BLOCK = 4;

// One launch of the sweep kernels covers sweeps [0, n_sweeps) of a call; trace / replay /
// schedule pointers are already offset to the launch's first sweep by the host.
struct SweepArgs {
    // couplings
    const void *J;           // dense: [n][ld] of float | int8, zero padded rows
    const int32_t *rowptr;   // CSR, layout entries < 2^31 (null otherwise)
    const long long *rowptr64;  // CSR, always present
    const uint32_t *cvp;     // CSR, slotted layout, packed entries (24-bit column | int8 value << 24) or null
    const int4 *rowinfo;     // CSR, slotted layout (rows padded to whole 64-entry slots), per row:
                             // first slot, slot count, slots from there to an all-zero slot, h (bits)
                             // in slots; the wide sweep forms address rows by it (null otherwise)
    const int2 *cv;          // CSR entries, (column, value bits) interleaved: one 8-byte load each
    const float *h;          // [n]
    const float *diag;       // [n] J_ii (ARITH_F32 only)
    // replica state
    int8_t *spins;           // [R][sstride], +-1, pad = 0
    double *energy;          // [R]
    double *best_energy;     // [R]
    int8_t *best_spins;      // [R][sstride]
    unsigned long long *n_accepted;  // [R]
    // temperatures
    const double *rep_temp;  // [R]
    const double *sched;     // optional T(k, r) = sched[k*sched_ss + r*sched_rs]
    long long sched_ss, sched_rs;
    // replay (parity tests)
    const int32_t *replay_site;  // [R][replay_stride], offset to this launch's first update
    const float *replay_u;
    long long replay_stride;
    // optional outputs
    double *energy_trace;        // [n_sweeps][R]
    uint8_t *accept_trace;       // [R][replay_stride]
    double *dE_trace;            // [R][replay_stride]
    long long ld;                // dense: spins per replica in LDS / HBM (= W * CPW * elems per chunk)
    long long ldj;               // dense: row stride of J in elements (n rounded up to 128 bytes)
    long long plane_bytes;       // bit-plane form: byte offset of the non-zero plane from the sign plane
    long long plane_row_bytes;   // bit-plane form: bytes of one row of one plane = round_up(n, 128) / 8
    int n, sstride, R, n_sweeps;
    int site_mode, arith, rule;
    // many-model batches (dense): replica r belongs to model (replica0 + r) / reps_per_model;
    // J / h / diag of model m start at m * model_stride_j / m * n elements (reps_per_model 0 = one model;
    // model_stride_j 0 with reps_per_model > 0 = one shared matrix under many field vectors, sga_set_dense_shared)
    // CSR launches: reps_per_model > 0 together with ragged == 0 means one set of rows under many field vectors
    // (sga_set_csr_shared): h of model m starts at m * n floats, rows and diag are the one model's; model_stride_j stays 0
    int reps_per_model;
    long long model_stride_j;
    int no_best;  // 1: leave best tracking to the host-driven pass (asymmetric / diagonal J)
    int table_m;  // > 0: J, h integer valued with max_i(sum_j |J_ij| + |h_i|) = table_m
    int table_scale;  // CSR: 1 | 2 -- table entry q stands for dE = 2 q / table_scale (2: J integer, h half-integer)
    int big;      // CSR: spins held as bits in LDS; 1 = one replica per workgroup with 64-bit row
                  // extents (n > ~160k, nnz >= 2^31, long rows), 2 = narrow form, several replicas per
                  // workgroup (short rows)
    int csr_acc;         // CSR: one of CSR_ACC_* (how a row sum is formed)
    int csr_head;        // CSR wide bit forms: head slots per wave the longest row needs (0: eight)
    int csr_pair_ahead;  // CSR narrow table form, every row <= 64 entries: 1 | 2 = the two updates of a pair reduced together
                         // (opt-in), 4 | 8 = that many updates per step, one per row of 16 | 8 lanes (sweep_csr_rows.hip)
    int csr_row_cap;     // CSR: entries of the longest row when that is <= 64 (else 0): sweep_csr_rows.hip picks its build by it
    int table_covers;    // CSR accept-table forms: 1 = no move of this problem lies beyond the table (scale * max_i(sum_j |J_ij| + |h_i|) <= table_m)
    int look_ahead;      // dense, integer problems: reduce LOOK updates together (sweep_dense_impl.h)
    int force_general;   // 1: the general kernel builds even for production arguments (engine option "force_general")
    int tsp_parallel;    // implicit TSP form: updates per step (-1: by the number of cities, 0 | 1: one at a time)
    // A launch over a SUBSET of the replicas (per-replica routing of SGA_FIELD_CACHE_AUTO): workgroup b works on
    // local replica rep_list[b], the grid covers rep_count of them (null: all R, workgroup b = replica b)
    const int *rep_list;
    int rep_count;
    const void *J_aux;   // bit-plane form: the int8 copy [n][ld] (single couplings for the look-ahead)
    // cached-local-field sweep (sweep_clf_impl.h): resident fields F = field_scale * (J s + h)
    void *fields;        // [R][ldf] int16 | int32
    long long ldf;
    int field_bits;      // 16 | 32; CSR: 0 = int16 fields, 32 | 64 = fixed-point fields (sweep_clf_csr.hip)
    int field_scale;     // 1 | 2 (J integer, h a multiple of 1/2); CSR fixed-point fields (sweep_clf_csr.hip): k, D = 2^k J s
    int clf_batched;     // 1: several accepts per round (sweep_clfb_impl.h) where the arguments are the production ones
    int clf_jmax;        // max |J_ij| (integer): the most one flip moves another site's field, in units of 2 scale
    // cached-field sweep of CSR problems (sweep_clf_csr.hip): fields = D [R][ldf] int16, D_i = sum_j J_ij s_j
    const int *clf_hq;   // [n] table_scale * h_i as integers (the static part of the local field)
    int clf_row_max;     // entries of the longest row of the layout (slot padding included)
    uint32_t seed_lo, seed_hi, sweep0, replica0;
    // ragged CSR batches (sga_set_csr_batch): replica r belongs to model (replica0 + r) / reps_per_model, whose
    // {first row in the concatenated CSR, spins} is entry m of an int2 table that starts `ragged` floats into h
    // (behind the models' fields, 8-byte aligned).  0: one model | dense batches (the fields above).  (An int, not a
    // pointer: it fills the struct's tail padding, so no other kernel's argument block changes.)
    int ragged;
};

// TSP-structured couplings that are never stored (sweep_tsp.hip): scaled distance tables + penalties
struct TspArgs {
    const float *nd4;    // [n_cities][npad]: -d[c][c']/4, zero diagonal, zero padded
    const float *nd4t;   // [n_cities][npad]: -d[c'][c]/4 as row c
    int n_cities, npad;  // npad = 256 * waves * passes >= n_cities (LDS column stride in bits, too)
    unsigned int div_magic;  // site / n_cities == (site * div_magic) >> 32 for every site (host verified)
    unsigned int row_bytes;  // 4 * npad
    float a2, b2;        // -A/2 (one position per city), -B/2 (one city per position)
    int f64;             // 0: integer instance, fp32 accumulation is exact; 1: fp64 accumulation
};
size_t tsp_lds_bytes(int n_cities, int npad);

// Couplings that are a sum of complete graphs on groups of sites, never stored (sweep_groups.hip, sga_set_groups)
struct GroupArgs {
    const int *gptr;              // [n + 1] site -> its memberships
    const int2 *gent;             // [gptr[n]] (group, coefficient bits) interleaved; never empty (one zero entry at least)
    const long long *member_ptr;  // [n_groups + 1] group -> its members
    const int *members;
    int n_groups;                 // >= 1 (0 only with a remainder)
    int wide;                     // 0: S_g as int16 in LDS (every group below 2^15 members) | 1: int32
    // the stored sparse remainder R of sga_set_groups_csr (J_ij = sum_g c_g + R_ij): symmetric, zero diagonal, rows
    // strictly sorted by column and at most GROUPS_MAX_REST_ROW long.  nnz == 0: no remainder, the REST = false kernels
    struct Rest {
        const int *rptr;   // [n + 1]
        const int2 *rent;  // [nnz] (column, value bits) interleaved
        long long nnz;
        int max_row;       // entries of the longest row
    } rest;
};
constexpr int GROUPS_MAX_MEMBERSHIPS = 64;  // groups one site may belong to (include/sga.h)
constexpr int GROUPS_MAX_REST_ROW = 256;    // entries of one remainder row (include/sga.h)
// per-row sum_j |R_ij| of a remainder (set-time bound of sga_set_groups_csr), one wave per row
hipError_t launch_groups_rest_row_abs(const long long *rowptr, const float *val, int n, double *out, hipStream_t st);
size_t groups_lds_bytes(int sstride, int n_groups, int wide);
size_t groups_energy_lds_bytes(int sstride, int n_groups, int wide);
hipError_t launch_sweep_groups(const SweepArgs &a, const GroupArgs &g, int waves, hipStream_t st);

// Wolff cluster rule (sweep_wolff.hip): recorded uniforms for the parity tests (null: Philox)
struct WolffArgs {
    const float *replay_u;   // [R][capacity], consumed in draw order from cursor[r]
    long long capacity;
    long long *cursor;       // [R]
};
size_t wolff_lds_bytes(int n);

struct EnergyArgs {
    int reps_per_model, replica_base;  // many-model batches, as in SweepArgs
    long long model_stride_j;
    const void *J;
    const long long *rowptr;
    const int2 *cv;
    const float *h;
    const int8_t *spins;
    double *energy;
    long long ld, ldj;
    int n, sstride, R;
    // The canonical order of X = sum_i mv_i s_i and Y = sum_i h_i s_i (energy_block_rows): `nblocks` blocks of
    // `block_rows` rows (TSP: of cities).  Few replicas: the blocks of one replica are cut into `slices` contiguous
    // ranges, one workgroup each (grid = R x slices); each block's (X, Y) sums land in partial[R][nblocks][2] and
    // launch_energy_finish adds them up in block order.  slices == 1: one workgroup per replica, same additions.
    int block_rows, nblocks;
    int slices, blocks_per_slice;  // slice y takes blocks [y bps, (y + 1) bps); every slice has some
    double *partial;
};
// Canonical order of a replica's energy sums, a function of n alone (so that its energy carries the same bits
// whatever the replica count, slicing, tiling or kernel of the launch): rows in blocks of energy_block_rows(n)
// (at most ENERGY_MAX_BLOCKS blocks); inside a block, chain c = 0..3 adds the terms of rows c, c + 4, ... in row
// order from 0; a block's sum is (c0 + c1) + (c2 + c3); X and Y add the block sums in block order, from 0.
constexpr int ENERGY_MAX_BLOCKS = 256;
__host__ __device__ inline int energy_block_rows(int n) {
    const int b = (n + ENERGY_MAX_BLOCKS - 1) / ENERGY_MAX_BLOCKS;
    return b > 8 ? b : 8;
}
// The CSR energy kernel with the replica's spins as bits in LDS (problems beyond the int8 LDS capacity) forms
// ENERGY_BITS_BLOCKS_PER_PASS blocks at a time: its slices take whole multiples of that.
constexpr int ENERGY_BITS_BLOCKS_PER_PASS = 4;
bool energy_csr_bits_form(int sstride);
// ragged CSR batches: replica r over the rows of model models[(replica_base + r) / reps_per_model] (one slice)
hipError_t launch_energy_csr_ragged(const EnergyArgs &a, const int2 *models, hipStream_t st);
hipError_t launch_energy_finish(const double *partial, int nblocks, int slices, double *energy, int R,
                                hipStream_t st);

// Local fields of all replicas in one pass over the couplings (fields_dense.hip, matrix cores)
struct FieldsArgs {
    const void *J;         // dense [n][ldj] int8 | float
    const int8_t *spins;   // [R][sstride]
    void *Y;               // [R][ldy] int32 (int8 J) | float: Y[r][i] = sum_j J[i][j] s[r][j]
    const float *h;        // [n]; many-model batches over one shared matrix: [n_models][n] (reps_per_model below)
    double *energy;        // [R] or null (finish pass)
    void *fields;          // [R][ldf] int16 | int32 or null (finish pass): field_scale * (Y + h)
    long long ldj, ldy, ldf;
    int n, R, sstride;
    int field_bits, field_scale;
    int eblock;  // energy_block_rows(n): the energies are summed in the per-replica kernels' order
    // sga_set_dense_shared (finish pass only): replica r of this tile is global replica replica_base + r and reads the h
    // of model (replica_base + r) / reps_per_model -- a tile may straddle models; 0 = one model
    int reps_per_model, replica_base;
};
// mode 0: int8 J (i8 MFMA) | 1: fp32 J with exact fp32 sums (f32 MFMA) | 2: fp32 J, real valued (f64 MFMA)
hipError_t launch_fields_dense(const FieldsArgs &a, int mode, hipStream_t st);
hipError_t launch_fields_finish(const FieldsArgs &a, bool y_is_int, hipStream_t st);
// cached-local-field sweep: dense integer-valued symmetric problems
hipError_t launch_sweep_clf(const SweepArgs &a, bool j_is_i8, int waves, hipStream_t st);
hipError_t launch_sweep_clfb(const SweepArgs &a, bool j_is_i8, int waves, hipStream_t st);  // several accepts per round
bool sweep_clfb_applies(const SweepArgs &a, bool j_is_i8);
size_t sweep_clfb_lds_bytes(long long ldf, int field_bits, int sstride, int table_m);
int sweep_clf_batch(long long ldj, bool j_is_i8, int waves);
// ... and of CSR problems with integer couplings (rows sorted, |sum_j J_ij s_j| < 2^15); a.field_bits = 32 | 64: the
// fixed-point form (option "clf_fixed_point"), D = 2^k J s with k = a.field_scale, no accept table
hipError_t launch_sweep_clf_csr(const SweepArgs &a, int waves, hipStream_t st);
bool sweep_clf_csr_applies(const SweepArgs &a, int waves);
size_t sweep_clf_csr_lds_bytes(long long ldf, int sstride, int table_m, int field_bits = 16);
hipError_t launch_csr_fields_seed(const long long *rowptr, const int2 *cv, const int8_t *spins, int sstride, int n, int R,
                                  short *D, long long ldf, hipStream_t st);
// D[r][i] = 2^k sum_j J_ij s_rj as int32 | int64 (field_bits), exact
hipError_t launch_csr_fields_seed_fx(const long long *rowptr, const int2 *cv, const int8_t *spins, int sstride, int n, int R,
                                     void *D, long long ldf, int field_bits, int k, hipStream_t st);
hipError_t launch_scaled_fields(const float *h, int n, int scale, int *hq, hipStream_t st);
// ... of ragged CSR batches (option "ragged_field_cache"): local replica r over the rows of model (replica0 + r) /
// reps_per_model; a workgroup takes up to eight replicas of ONE model (models[] = {first row, spins}, on the device)
hipError_t launch_csr_fields_seed_ragged(const long long *rowptr, const int2 *cv, const int8_t *spins, int sstride, int n_max,
                                         int R, unsigned int replica0, int reps_per_model, const int2 *models, short *D,
                                         long long ldf, hipStream_t st);
// ... with fixed-point fields (options "ragged_field_cache" and "clf_fixed_point" together): D = 2^k J_m s as int32 | int64,
// one k and one width for the batch
hipError_t launch_csr_fields_seed_ragged_fx(const long long *rowptr, const int2 *cv, const int8_t *spins, int sstride, int n_max,
                                            int R, unsigned int replica0, int reps_per_model, const int2 *models, void *D,
                                            long long ldf, int field_bits, int k, hipStream_t st);
// ... and of dense problems with real-valued J (option "clf_fixed_point", sweep_clf_fx.hip): D = 2^k J s as exact int32 |
// int64 (a.field_bits), k = a.field_scale, no accept table; fp32 rows, or int8 rows (integer J, k = 0)
// (a.reps_per_model > 0: the build for many-model batches, option "batch_fixed_point" -- n_models names the batch in the
//  kernel note)
hipError_t launch_sweep_clf_fx(const SweepArgs &a, bool j_is_i8, int waves, hipStream_t st, int n_models = 1);
// ... the seed of a many-model batch: local replica r over the rows of model (replica0 + r) / reps_per_model, exact fp64
// sums at the batch-wide k, one launch whatever the number of models
hipError_t launch_dense_fields_seed_fx_batch(const void *J, bool j_is_i8, long long ldj, long long model_stride_j,
                                             const int8_t *spins, int sstride, int n, int R, unsigned int replica0,
                                             int reps_per_model, void *D, long long ldf, int field_bits, int k, hipStream_t st);
bool sweep_clf_fx_applies(const SweepArgs &a, bool j_is_i8);
size_t sweep_clf_fx_lds_bytes(long long ldf, int field_bits, int sstride);
// D[r][i] = 2^k sum_j J_ij s_rj as int32 | int64 (field_bits), exact; J dense [n][ldj] fp32 | int8
hipError_t launch_dense_fields_seed_fx(const void *J, bool j_is_i8, long long ldj, const int8_t *spins, int sstride, int n,
                                       int R, void *D, long long ldf, int field_bits, int k, hipStream_t st);
// F[r][i] = scale (J_m s_r + h_m)[i] as int16 | int32 (field_bits) for the local replicas of a many-model batch, m =
// (replica0 + r) / reps_per_model: exact integer sums, one launch whatever the number of models (sweep_clf.hip)
hipError_t launch_dense_fields_seed_batch(const void *J, bool j_is_i8, long long ldj, long long model_stride_j, const float *h,
                                          const int8_t *spins, int sstride, int n, int R, unsigned int replica0,
                                          int reps_per_model, void *F, long long ldf, int field_bits, int scale,
                                          hipStream_t st);
size_t sweep_clf_lds_bytes(long long ldf, int field_bits, int sstride, int table_m);
int sweep_clf_waves(long long ldj, bool j_is_i8, int R, int cus, int forced);

// Energies of all replicas of a CSR problem in one pass over the entries (fields_csr.hip)
struct CsrEnergyArgs {
    const long long *rowptr;
    const int2 *cv;
    const unsigned int *sb;  // [n][RW] transposed spin bits
    double *partial;         // [groups][32 RW]
    int n, R, RW, groups;
};
// (h . s in the canonical order; X in group order, the same bits only where it is exact: sga_engine.cpp)
size_t csr_energy_scratch_bytes(int n, int R, int groups);
// (reps_per_model > 0: one set of rows under many field vectors, h [n_models][n] -- replica r of this pass is global
//  replica replica_base + r and takes the h of model (replica_base + r) / reps_per_model; the pass over the entries is
//  the same one, whatever the models of the 32 replicas a lane carries)
hipError_t launch_energy_csr_all(const long long *rowptr, const int2 *cv, const float *h, const int8_t *spins, int sstride,
                                 int n, int R, int groups, bool exact32, void *scratch, double *energy, hipStream_t st,
                                 int reps_per_model = 0, int replica_base = 0);

struct ExchangeArgs {
    const double *energies;   // [R_global] by global replica id
    const double *slot_temps; // [R_global]
    int32_t *slot_to_rep;     // [R_global]
    double *rep_temp;         // [R_local]
    long long *attempts, *accepts;  // [R_global] indexed by lower slot of the pair
    const int32_t *start;     // [n_ladders] or null
    const double *u;          // [n_ladders][L/2] or null
    int *n_accepted;          // device counter
    int R_global, R_local, replica0, n_ladders;
    uint32_t seed_lo, seed_hi, round;
    // the ladders this launch decides: all of them (energies by global id), or only those the local replicas fill
    // (whole ladders per rank: `energies` are the local ones, shifted by energy_base = replica0; no gather needed)
    int ladder0, n_ladders_local, energy_base;
};

// launchers (defined in the .hip files); all return hipGetLastError() after the launch
hipError_t launch_sweep_dense(const SweepArgs &a, bool j_is_i8, int acc64, int waves, int cpw,
                              hipStream_t st);  // acc64: 0 fp32 | 1 fp64 any order (exact) | 2 fp64 canonical
// updates reduced together by the production sweeps of an integer problem with this layout (1 =
// one at a time): sweep_dense_impl.h, look-ahead form
int dense_look_ahead(bool t2, bool j_is_i8, bool acc64, int cpw, int waves, int R);
// ternary couplings as two bit-planes (production configuration only)
hipError_t launch_sweep_dense_t2(const SweepArgs &a, int waves, int cpw, hipStream_t st);
// fp32 [n][n] -> sign plane + non-zero plane, each [n][row_bits/32] words, plus nnz[n] (as float)
hipError_t launch_repack_tern2(const float *J, long long ldJ, int n, unsigned int *planes,
                               long long row_bits, float *row_nnz, hipStream_t st);
hipError_t launch_sweep_csr(const SweepArgs &a, int waves_per_replica, hipStream_t st);
bool sweep_csr_rows_applies(const SweepArgs &a);  // sweep_csr_rows.hip: four | eight updates per step
hipError_t launch_sweep_csr_rows(const SweepArgs &a, int waves_per_block, hipStream_t st);
hipError_t launch_sweep_wolff(const SweepArgs &a, const WolffArgs &wa, bool csr, bool j_is_i8, hipStream_t st);
hipError_t launch_sweep_tsp(const SweepArgs &a, const TspArgs &t, int waves, int passes, hipStream_t st);
hipError_t launch_energy_tsp(const EnergyArgs &a, const TspArgs &t, hipStream_t st);
hipError_t launch_fields_tsp(const TspArgs &t, const int8_t *spins, const float *h, const int32_t *sites,
                             int count, double *out, hipStream_t st);
hipError_t launch_energy_groups(const EnergyArgs &a, const GroupArgs &g, hipStream_t st);
hipError_t launch_fields_groups(const GroupArgs &g, const int8_t *spins, const float *h, const int32_t *sites, int count,
                                double *out, hipStream_t st);
hipError_t launch_tsp_tables(const float *d, long long ldd, int n, int npad, float *nd4, float *nd4t,
                             hipStream_t st);
int csr_waves_per_block(int sstride, int table_m);  // replicas per workgroup that fit LDS (0: none)
bool csr_big_fits(int sstride, int table_m);         // spins as bits: one replica per workgroup
int csr_bits_waves_per_block(int sstride, int table_m);  // spins as bits, narrow form: replicas per workgroup
size_t csr_lds_bytes(int sstride, int table_m, bool bits);  // LDS of one replica (spins + table)
hipError_t launch_energy_dense(const EnergyArgs &a, bool j_is_i8, hipStream_t st);
hipError_t launch_energy_csr(const EnergyArgs &a, hipStream_t st);
hipError_t launch_exchange_neighbor(const ExchangeArgs &a, hipStream_t st);
// ordered list of slot pairs [count][2], one serial chain (exchange_method="all_pairs")
hipError_t launch_exchange_pairs(const ExchangeArgs &a, const int32_t *pairs, int count, hipStream_t st);
hipError_t launch_init_spins(int8_t *spins, int n, int sstride, int R, uint32_t seed_lo,
                             uint32_t seed_hi, uint32_t replica0, hipStream_t st);
// J repack: fp32 [n][ldJ] -> float | int8 [n][ld] zero padded (ld = the packed row stride), plus diag[n]
hipError_t launch_repack_dense(const float *J, long long ldJ, long long rows, int n, void *out,
                               long long ld, bool to_i8, float *diag, hipStream_t st);
// flags[0] = 1 if some J is not an integer in [-127,127]; flags[1] = 1 if some J is outside
// {-1, 0, +1} (ternary couplings can be held as two bit-planes)
// ... flags[5] = 1024 + highest binary exponent of a non-zero value, flags[6] = 1024 - exponent of
// the lowest set bit (0: no non-zero value): is the fp64 sum of a row exact in any order?
hipError_t launch_scan_values(const float *v, long long rows, long long cols, long long ld,
                              int *flags, hipStream_t st);
// ragged CSR batches: replica r as a one-model engine of models[(replica0 + r) / reps].y spins would draw it
hipError_t launch_init_spins_ragged(int8_t *spins, int sstride, int R, uint32_t seed_lo, uint32_t seed_hi,
                                    uint32_t replica0, const int2 *models, int reps, hipStream_t st);
// ... and the padding past each replica's model zeroed (spins handed over as [R][n_max])
hipError_t launch_mask_spins_ragged(int8_t *spins, int sstride, int R, uint32_t replica0, const int2 *models,
                                    int reps, hipStream_t st);
hipError_t launch_pad_spins(const int8_t *src, int n, int8_t *dst, int sstride, int R,
                            hipStream_t st);
hipError_t launch_unpad_spins(const int8_t *src, int sstride, int8_t *dst, int n, int R,
                              hipStream_t st);
hipError_t launch_gather_diag_csr(const long long *rowptr, const int32_t *colidx, const float *val,
                                  int n, float *diag, hipStream_t st);
// (colidx, val) -> interleaved entries {column, value bits}: a row is one stream of 8-byte loads
// (half the memory instructions, one page instead of two per row)
hipError_t launch_pack_cv(const int32_t *colidx, const float *val, int2 *cv, long long nnz,
                          hipStream_t st);
// row-wise packing into a (possibly padded) layout; cv_src != null: re-pad an interleaved layout
hipError_t launch_pack_cv_rows(const long long *src_ptr, const long long *dst_ptr, const int32_t *colidx,
                               const float *val, const int2 *cv_src, int2 *cv, int n, hipStream_t st);
// CSR row extents between their 32- and 64-bit forms ([n + 1] entries)
hipError_t launch_widen_rowptr(const int32_t *src, long long *dst, long long count, hipStream_t st);
hipError_t launch_rowinfo_fields(int4 *rowinfo, const float *h, int n, hipStream_t st);
hipError_t launch_pack_entries(const int2 *cv, uint32_t *cvp, long long count, int *bad, hipStream_t st);
hipError_t launch_narrow_rowptr(const long long *src, int32_t *dst, long long count, hipStream_t st);
// CSR structure checks on the device.  flags (int[CSR_FLAG_COUNT] = int[10], zeroed by the caller):
//  [0] rowptr not monotone / not spanning [0, nnz]   [1] column out of range
//  [2] value bits (below)                             [3] rows not strictly sorted by column
//  [4] non-zero diagonal entry                        [5] J[i][j] != J[j][i]
//  [6] bits of max_i(sum_j |J_ij| + |h_i|) as float
//  [7] 1024 + exponent of the highest set bit of any non-zero J (subnormals: their true top bit)
//  [8] 1024 - exponent of the lowest set bit          [9] bits of max_i sum_j |J_ij| as float
//  ([2]: bit 0 = some J not an integer, bit 1 = some h not an integer, bit 2 = some h not a multiple of 1/2,
//   bit 3 = SCAN_NON_FINITE: some J or h is NaN or +-Inf -- the setters refuse the problem; [6] to [9] then mean nothing)
// The dense scans (launch_scan_values / launch_dense_row_abs_max) keep the same four bits in their word [3].
enum { SCAN_NON_FINITE = 8 };
enum { CSR_BAD_ROWPTR = 0, CSR_BAD_COLUMN, CSR_NOT_INTEGRAL, CSR_UNSORTED, CSR_DIAGONAL,
       CSR_ASYMMETRIC, CSR_ROW_ABS_MAX, CSR_EXP_HI, CSR_EXP_LO, CSR_ROW_J_ABS_MAX, CSR_FLAG_COUNT = 10 };
// how the CSR sweep kernels form a row sum
enum { CSR_ACC_F32_TABLE = 0,   // integer J and h, few distinct uphill moves: fp32 (exact) + accept table
       CSR_ACC_F32 = 1,         // integer J with row sums below 2^24: fp32 accumulation is exact
       CSR_ACC_F64 = 2,         // the fp64 sum of the row's fp32 values is exact (binary exponents of
                                // all J within 53 bits of each other incl. the row length): any order
       CSR_ACC_F64_CANON = 3 }; // anything else: fp64 in the canonical order (sweep_csr.hip)
hipError_t launch_csr_check_rowptr(const long long *rowptr, int n, long long nnz, int *flags,
                                   hipStream_t st);
hipError_t launch_csr_scan(const long long *rowptr, const int32_t *colidx, const float *val,
                           const float *h, int n, int *flags, hipStream_t st, int n_h = 1);
// sorted = rows strictly sorted by column (binary search); else linear scans of both rows
hipError_t launch_csr_symmetry(const long long *rowptr, const int32_t *colidx, const float *val,
                               int n, bool sorted, int *flags, hipStream_t st);
hipError_t launch_copy_best(const double *energy, const int8_t *spins, double *best_energy,
                            int8_t *best_spins, int sstride, int R, hipStream_t st);

// *out += position-weighted checksum of the 32-bit words of buf (sga_problem_checksum)
hipError_t launch_checksum(const void *buf, long long bytes, unsigned long long *out, hipStream_t st);
// streaming read of `bytes` (a multiple of 16) of device memory, for the bandwidth probe
hipError_t launch_probe_read(const void *buf, long long bytes, float *sink, hipStream_t st);

// single-site operators (IsingModel.get_local_field / flip_spin, SpinDynamics.single_spin_update)
struct PointArgs {
    const void *J;
    const long long *rowptr;
    const int2 *cv;
    const float *h, *diag;
    int8_t *spins;       // the replica's row [sstride]
    double *energy;      // the replica's tracked energy
    unsigned long long *n_accepted;
    const int32_t *sites;  // [count]
    double *out;           // [count] fields (op 0) | out[0] = dE, out[1] = accepted (ops 1, 2)
    long long ld, ldj;
    int n, count, op;      // op 0: fields, 1: flip, 2: metropolis
    int arith, rule;
    double T;
    float u;
    long long model_offset_j;  // element offset of this replica's model in J; h/diag pre-offset
};
hipError_t launch_point_op(const PointArgs &a, bool csr, bool j_is_i8, hipStream_t st);

// 1 -> out[0] if some J[i][j] != J[j][i] or J[i][i] != 0 (per model block of n rows)
hipError_t launch_check_symmetric(const float *J, long long ldJ, long long rows, int n, int *out,
                                  hipStream_t st);
// best[r] = min(best[r], energy[r]) with the spins, one workgroup per replica
hipError_t launch_update_best(const double *energy, const int8_t *spins, double *best_energy,
                              int8_t *best_spins, int sstride, int R, hipStream_t st);

// Row-shared windows (sweep_dense_rs.hip): the dense sweep of integer problems with one coupling-row read per
// proposed site and window of W updates per replica.  Scratch of the window plan and the fields, and the problem's
// resident bit-planes of J (owned by the engine, made once per problem):
struct RowSharedPlan {
    int *cnt;        // [n_windows][n_groups][n] proposals per (window, replica group, site); after the scan the first
                     // entry of each (the fill's cursors)
    int *off;        // [n_windows][n + 1] first entry of each (window, site)
    int *tot;        // [n_windows][row_shared_scan_chunks(n)] proposals per (window, chunk of 1024 sites): the scan's carries
    int *ent;        // [R n] (replica << log_w | update in window), grouped by (window, site)
                     // The tile kernel's plan (rs_tile_plan_kernel) in the same two arrays: ent grouped by (window, slice
                     // of replicas, tile, replica), site in tile | replica in slice << 12 | update in window << 17; cnt
                     // as 16-bit words [n_windows][tiles][slices], the first entry of each run inside its slice
    int *base;       // [R][W] row sums against the window-start spins
    uint32_t *bits;  // [R][nw32] window-start spins, 1 = down (the layout of sweep_dense_rs.hip)
    const unsigned long long *jp;  // [n][planes + 1][nw32 / 2] sign plane and magnitude planes of every row of J in the
                                   // spins' bit layout; null: the fields kernel converts the rows of J on chip
    const int *jabs;               // [n] sum_j |J_ij| (with jp)
    int W, log_w, nw32, planes;  // planes: magnitude bit-planes of |J| (1 | 3 | 8)
    int log_rg, n_groups;        // replicas per group of the plan (a power of two), groups
};
// What the GRID instantiations take instead (option "row_shared_grid"): the planes hold 2^k J, the chain works in real
// units and decides with the row kernels' general rule.  A type of its own, so that the kernels of the integer form
// keep their arguments byte for byte.
struct RowSharedGridPlan {
    RowSharedPlan p;
    int k;
};
// magnitude bit-planes of |J| for an integer bound on it; 0: |J| beyond 255, the form does not apply
inline int row_shared_planes(int j_abs_max) { return j_abs_max <= 1 ? 1 : j_abs_max <= 7 ? 3 : j_abs_max <= 255 ? 8 : 0; }
inline int row_shared_nw32(int n) { return 8 * ((n + 255) / 256); }
inline int row_shared_scan_chunks(int n) { return (n + 1023) / 1024; }  // workgroups of the scan per window
// Resident planes exist where they take at most half the bytes of J: fp32 rows always ((planes + 1) / 32 of J), int8
// rows for 1 and 3 magnitude planes; int8 rows with 8 planes keep the on-chip conversion.
inline bool row_shared_resident(bool j_is_i8, int planes) { return planes > 0 && (!j_is_i8 || planes <= 3); }
inline size_t row_shared_plane_bytes(int n, int planes) {
    return (size_t)n * (size_t)(planes + 1) * (size_t)(row_shared_nw32(n) / 2) * 8;
}
// log2 of the replicas per group of the window plan: at least 32, and at least the number of windows, so that a slice
// (one window, one group: W 2^log_rg entries) holds about as many entries as its histogram has sites and the counts
// stay within the bytes of the entries
inline int row_shared_log_group(int n, int W) {
    const int nwin = (n + W - 1) / W;
    int l = 5;
    while ((1 << l) < nwin) ++l;
    return l;
}
// The chain's accept table (rs_chain_kernel, integer Metropolis form): a wave tabulates ptab[q] = expf_det((float)(
// -(double)(2 q) / T)), q = 1 ... Q, once per window and decides u < ptab[q] from LDS.  Q = min(table_m,
// RS_ACCEPT_TABLE_MAX, zero_from(T)), zero_from(T) = floor(52 T) + 2 where 0 <= 52 T < RS_ACCEPT_TABLE_MAX and no bound
// otherwise (T < 0, inf, NaN).  Where Q == zero_from(T) every q > Q is decided "false" without an entry:
//   * fl(52 T) >= k whenever 52 T >= k for an integer k (k is an fp64 number, rounding is monotone), so floor(fl(52 T))
//     >= floor(52 T) and q >= floor(52 T) + 3 > 52 T + 2, that is 2 q > 104 T + 4;
//   * T > 0: the quotient -(2 q) / T < -104 - 4 / T < -104; -104 is an fp64 and an fp32 number, so neither the rounding
//     of the divide nor the conversion to fp32 (both monotone) lifts the argument above -104, and expf_det returns 0
//     below -103.972084; no uniform u >= 0 is below 0.  (q > table_m: rs_accept's cut-off 2 q > fl(104 T) holds by the
//     margin of 4 against a rounding error of 104 T 2^-53, T < 20 -- false as well.)
//   * T = 0: zero_from = 2, the quotient is -inf for every q >= 1, expf_det(-inf) = 0: false, as the entries 1 and 2 are.
// Elsewhere (Q at the cap, or cut by table_m) a q > Q takes rs_accept's own per-lane evaluation.
constexpr int RS_ACCEPT_TABLE_MAX = 1023;  // entries 0 ... 1023: 4 KB of floats per chain wave
__host__ __device__ inline int rs_accept_table_zero_from(double T) {
    const double x = 52.0 * T;
    return (x >= 0.0 && x < (double)RS_ACCEPT_TABLE_MAX) ? (int)x + 2 : 0x7fffffff;  // ((int)x: floor, x >= 0)
}
__host__ __device__ inline int rs_accept_table_entries(double T, int table_m) {
    const int z = rs_accept_table_zero_from(T);
    int Q = table_m < RS_ACCEPT_TABLE_MAX ? table_m : RS_ACCEPT_TABLE_MAX;
    if (Q < 0) Q = 0;
    return z < Q ? z : Q;
}
// Fields from the resident planes in tiles (rs_fields_tiles_kernel, option "row_shared_fields"): one workgroup per
// (window, tile of S consecutive sites) holds the tile's plane rows in LDS and walks its entries grouped by replica.
// S == 0: the per-site kernel.  ones: every off-diagonal |J_ij| (GRID: |2^k J_ij|) is 1 -- the rows are their sign
// planes alone ("sign-only").  A type of its own beside the plan, so that the other kernels keep their arguments.
struct RowSharedTiles {
    int S = 0;
    int ones = 0;
};
constexpr int RS_TILE_THREADS = 1024;        // workgroup of the tile kernel
constexpr int RS_TILE_ENTRIES = 6144;        // its entry buffer: a longer range goes through in chunks of this many
constexpr int RS_TILE_MAX_REPLICAS = 4096;   // its replica counters (one LDS word per replica of the launch)
constexpr int RS_TILE_MAX_SITES = 4096;      // (a site's index in the tile is kept in 16 bits)
constexpr size_t RS_TILE_LDS_BUDGET = 160 * 1024 - 256;
// Option "row_shared_fields" = 2 takes the tiles only where a replica's spin bits are at least this many bytes (n > 7936):
// what a tile saves is bits per entry, what it costs -- the sort -- is per entry whatever n.  Measured at 1024 replicas,
// W = 1024: 1280 B (n = 10 000) 67.5 -> 57.0 us per window, 256 B (n = 2000) 30.7 -> 34.3 us; the straight line between
// the two crosses at about 520 B, and the default asks for twice that.
constexpr int RS_TILE_MIN_BITS_BYTES = 1024;
// 16-byte words of a replica's spin bits that a lane of the tile kernel keeps in registers (a quarter wave holds 256 bytes
// per word: n <= 16384 beside one magnitude plane); longer vectors, and eight planes, stream the bits per entry
constexpr int row_shared_tile_register_words(int planes) { return planes == 1 ? 8 : planes == 3 ? 4 : 0; }
// Option "row_shared_fields" = 2: null where the tiles are the default -- the one configuration measured to win, sign-only
// rows with the bits in registers from RS_TILE_MIN_BITS_BYTES (7936 < n <= 16384) -- else why the per-site kernel runs.
// General planes measured slower or level in tiles; option 1 takes the tiles wherever they can run.
inline const char *row_shared_tiles_not_default(int n, int planes, bool ones) {
    const int bytes = 4 * row_shared_nw32(n);
    if (!ones) return "rows not sign-only; row_shared_fields = 1 forces the tiles";
    if (bytes < RS_TILE_MIN_BITS_BYTES) return "spin bits under 1 KB per replica: the per-site kernel is faster";
    if (bytes > 256 * row_shared_tile_register_words(planes))
        return "spin bits beyond the kernel's registers; row_shared_fields = 1 forces the tiles";
    return nullptr;
}
// dynamic LDS of the tile kernel: [S][rows per site][nw32 / 4] 16-byte words of planes, the sorted entries (32-bit
// entry, 16-bit site in the tile), R counters, S + 1 offsets, S row constants, one total per wave
inline size_t row_shared_tile_lds(int n, int planes, bool ones, int S, int R) {
    const size_t row = (size_t)(ones ? 1 : planes + 1) * (size_t)row_shared_nw32(n) * 4;
    return (size_t)S * row + (size_t)RS_TILE_ENTRIES * 6 + 4 * ((size_t)R + 2 * (size_t)S + 1 + RS_TILE_THREADS / 64);
}
// The tile size for a problem and replica count, 0 where the per-site kernel serves (why: the reason).  forced > 0:
// option "row_shared_tile_sites".  The rule: S = ceil(n / (m cus)) for the smallest m whose image fits LDS, at least 2
// -- ceil(n / S) tiles then fill m rounds of one workgroup per CU almost whole.
inline int row_shared_tile_sites(int n, int planes, bool ones, int R, int cus, int forced, const char **why) {
    const char *dummy;
    if (!why) why = &dummy;
    *why = nullptr;
    if (planes <= 0 || n <= 0) return (*why = "no resident bit-planes"), 0;
    if (R > RS_TILE_MAX_REPLICAS) return (*why = "more replicas than the tile kernel's 4096 LDS counters"), 0;
    if (row_shared_tile_lds(n, planes, ones, 2, R) > RS_TILE_LDS_BUDGET) return (*why = "two rows' planes do not fit the tile image in LDS"), 0;
    if (forced > 0) {
        const int S = forced < 2 ? 2 : forced > RS_TILE_MAX_SITES ? RS_TILE_MAX_SITES : forced;
        if (row_shared_tile_lds(n, planes, ones, S, R) > RS_TILE_LDS_BUDGET) return (*why = "the forced tile does not fit LDS"), 0;
        return S;
    }
    if (cus <= 0) cus = 256;
    for (long long m = 1;; ++m) {
        long long S = ((long long)n + m * cus - 1) / (m * cus);
        if (S < 2) S = 2;
        if (S <= RS_TILE_MAX_SITES && row_shared_tile_lds(n, planes, ones, (int)S, R) <= RS_TILE_LDS_BUDGET) return (int)S;
    }
}
// The plan of the tile kernel (rs_tile_plan_kernel): a workgroup owns a slice -- one window, rg consecutive replicas -- and
// sorts its rg W entries in LDS by (tile, replica); it asks for rg W words of staging, a counter per (tile of its pass,
// replica), and RS_TILE_PLAN_EXTRA words.  The first entry of every (window, tile, slice) run goes, 16 bits wide (at most
// 32 W), where the by-site plan keeps its counts: ceil(n / S) ceil(R / rg) values per window must fit the n ceil(R / 2^
// row_shared_log_group) words the engine allocates there.  rg: a power of two, at most 32 (5 bits of the entry word), 0
// where no geometry serves; tiles: the tiles a workgroup covers in one pass -- fewer than ceil(n / S) where the tiles
// are covered in ranges, every range walking the slice's Philox blocks again (a third grid dimension).
struct RowSharedTilePlan {
    int rg = 0;
    int tiles = 0;
};
constexpr int RS_TILE_PLAN_THREADS = 1024;      // workgroup of the plan
constexpr int RS_TILE_PLAN_EXTRA = 32;          // words beside staging and counters: the scan's wave totals, two sums
constexpr size_t RS_TILE_PLAN_LDS = 80 * 1024;  // what the rule asks for: two workgroups per CU
inline size_t row_shared_tile_plan_lds(int W, int rg, int tiles) {
    return 4 * ((size_t)rg * (size_t)W + (size_t)rg * (size_t)tiles + RS_TILE_PLAN_EXTRA);
}
inline bool row_shared_tile_plan_runs_fit(int n, int W, int S, int R, int rg) {
    const long long ntiles = (n + S - 1) / S, slices = (R + rg - 1) / rg;
    const long long groups = ((long long)R + (1ll << row_shared_log_group(n, W)) - 1) >> row_shared_log_group(n, W);
    return 2 * ntiles * slices <= 4 * groups * (long long)n;
}
// The rule: the largest rg whose staging and counters for ALL tiles fit RS_TILE_PLAN_LDS (and whose run starts fit);
// else tile ranges with the smallest rg whose run starts fit -- the fewest ranges, so the fewest walks of the Philox
// blocks -- in RS_TILE_PLAN_LDS, and last in the tile kernel's own budget (32 replicas of W = 1024 stage 128 KB).
inline RowSharedTilePlan row_shared_tile_plan(int n, int W, int S, int R) {
    RowSharedTilePlan t;
    if (n <= 0 || S <= 0 || R <= 0 || W <= 0) return t;
    const int ntiles = (n + S - 1) / S;
    for (int rg = 32; rg >= 1; rg >>= 1)
        if (row_shared_tile_plan_lds(W, rg, ntiles) <= RS_TILE_PLAN_LDS && row_shared_tile_plan_runs_fit(n, W, S, R, rg))
            return (t.rg = rg), (t.tiles = ntiles), t;
    const size_t budgets[2] = {RS_TILE_PLAN_LDS, RS_TILE_LDS_BUDGET};
    for (const size_t budget : budgets)
        for (int rg = 1; rg <= 32; rg <<= 1) {
            if (row_shared_tile_plan_lds(W, rg, 1) > budget || !row_shared_tile_plan_runs_fit(n, W, S, R, rg)) continue;
            const size_t per_pass = (budget / 4 - RS_TILE_PLAN_EXTRA - (size_t)rg * (size_t)W) / (size_t)rg;
            return (t.rg = rg), (t.tiles = per_pass < (size_t)ntiles ? (int)per_pass : ntiles), t;
        }
    return t;
}
// Replica groups (launch_sweep_dense_rs over the tile plan): replicas are independent inside a sweep, so contiguous ranges
// of them run the whole sweep -- plan, (fields, chain) per window, best tracking -- as engines of their own on streams of
// their own: the chain of one group fills the SIMD slots beside the fields of another, no kernel waits on another group,
// and a replica's chain is the one-group chain (every launch of a group takes the group's own SweepArgs and plan view;
// the device code knows nothing of groups).  The rule: (R, G asked for) -> at most G ascending, disjoint, non-empty ranges
// [begin[g], begin[g + 1]) that cover [0, R); every inner boundary is a multiple of 32, the largest slice of the tile
// plan, so that no slice straddles two groups.  R <= 32: one group.
constexpr int RS_MAX_GROUPS = 4;  // with the caller's stream: within the four hardware queues a process gets by default
struct RowSharedGroups {
    int G = 1;
    int begin[RS_MAX_GROUPS + 1] = {0, 0, 0, 0, 0};
};
inline RowSharedGroups row_shared_groups(int R, int G) {
    RowSharedGroups g;
    g.begin[1] = R > 0 ? R : 0;
    if (R <= 32 || G <= 1) return g;
    const int slices = (R + 31) / 32;
    g.G = G > RS_MAX_GROUPS ? RS_MAX_GROUPS : G;
    if (g.G > slices) g.G = slices;
    for (int i = 1; i < g.G; ++i) g.begin[i] = 32 * (int)((long long)slices * i / g.G);
    g.begin[g.G] = R;
    return g;
}
// What a group's view of the plan's scratch starts at, in elements of each array (RowSharedPlan): ent, base and bits are
// per replica; cnt is carved by the by-site plan's own unit, n words per window and group of 2^row_shared_log_group
// replicas -- the share a one-group engine of R_g replicas would have allocated, inside which row_shared_tile_plan finds
// room for its run starts (row_shared_tile_plan_runs_fit asks exactly that of R_g).
struct RowSharedGroupView {
    long long cnt = 0, ent = 0, base = 0, bits = 0;
    int n_groups = 0;  // plan groups of the view: ceil(R_g / 2^log_rg)
};
inline RowSharedGroupView row_shared_group_view(int n, int W, const RowSharedGroups &g, int i) {
    const int l = row_shared_log_group(n, W);
    const long long nwin = (n + W - 1) / W;
    RowSharedGroupView v;
    long long before = 0;
    for (int j = 0; j < i; ++j) before += ((long long)(g.begin[j + 1] - g.begin[j]) + (1ll << l) - 1) >> l;
    v.cnt = nwin * before * n;
    v.ent = (long long)g.begin[i] * n;
    v.base = (long long)g.begin[i] * W;
    v.bits = (long long)g.begin[i] * row_shared_nw32(n);
    v.n_groups = (int)(((long long)(g.begin[i + 1] - g.begin[i]) + (1ll << l) - 1) >> l);
    return v;
}
// Whether G groups can run: every group's tile plan exists for its R_g (its run starts inside its share of cnt), and the
// shares together stay inside the allocation of the R replicas (beyond 32 windows a plan group is more than 32 replicas
// and the shares of ranges cut at multiples of 32 may round up past it).  Else: one group.
inline bool row_shared_groups_fit(int n, int W, int S, int R, const RowSharedGroups &g) {
    if (g.G <= 1) return true;
    if (n <= 0 || W <= 0 || S <= 0) return false;
    const int l = row_shared_log_group(n, W);
    long long shares = 0;
    for (int i = 0; i < g.G; ++i) {
        const int Rg = g.begin[i + 1] - g.begin[i];
        if (Rg <= 0 || row_shared_tile_plan(n, W, S, Rg).rg <= 0) return false;
        shares += ((long long)Rg + (1ll << l) - 1) >> l;
    }
    return shares <= (((long long)R + (1ll << l) - 1) >> l);
}
// The default count: the largest of RS_DEFAULT_MAX_GROUPS, ..., 2, 1 that leaves every group at least RS_GROUP_MIN_REPLICAS
// replicas.  Both from measurements at n = 10 000, W = 1024 over 64 ... 2048 replicas: two groups win from
// 2 x 256 replicas and are level at 2 x 128; below, the tile kernel's fixed cost per launch -- a tile's rows, the prefix
// over the runs -- outweighs what the overlap saves.  Four groups lost to two at every count measured (groups of 16 to 512
// replicas): a CU holds one workgroup of the tile kernel (its LDS), so the fields launches of the groups queue behind each
// other and every chain waits for its own; four stay behind the setter.
constexpr int RS_GROUP_MIN_REPLICAS = 256;
constexpr int RS_DEFAULT_MAX_GROUPS = 2;
inline int row_shared_default_groups(int R) {
    for (int G = RS_DEFAULT_MAX_GROUPS; G > 1; G >>= 1) {
        const RowSharedGroups g = row_shared_groups(R, G);
        bool ok = g.G == G;
        for (int i = 0; i < g.G; ++i) ok = ok && g.begin[i + 1] - g.begin[i] >= RS_GROUP_MIN_REPLICAS;
        if (ok) return G;
    }
    return 1;
}
// The streams and events of a grouped launch (the engine's: made once, destroyed with it): group 0 runs on the launch's
// stream, group g > 0 on stream[g - 1]; one fork at the start of the call, one join per group at its end.
struct RowSharedGroupRun {
    int G = 1;  // groups asked of row_shared_groups (the launch refuses a count that does not fit)
    hipStream_t stream[RS_MAX_GROUPS - 1] = {nullptr, nullptr, nullptr};
    hipEvent_t fork = nullptr, join[RS_MAX_GROUPS - 1] = {nullptr, nullptr, nullptr};
};
// asks the runtime for the tile kernel's LDS (once per instantiation and size): an error where it is refused
hipError_t row_shared_tiles_prepare(int planes, bool ones, size_t lds_bytes);
// one pass over J: jp and jabs of every row (the first time the form is prepared for a problem); grid_k: the planes
// and jabs are those of 2^k J (fp32 rows; 0: of J itself)
hipError_t launch_rs_build_planes(const void *J, bool j_is_i8, long long ldj, int n, int planes, int grid_k,
                                  unsigned long long *jp, int *jabs, hipStream_t st);
// a.n_sweeps sweeps: spins -> bits, then per sweep the plan, per window fields + chain, best tracking.  Production
// arguments only (Philox sites, fp64 rule, no per-update traces, all replicas).  a.rule: Metropolis decides with the
// accept table; Glauber and heat bath with the row kernels' general rule (the ANYRULE instantiations, "rule=glauber" /
// "rule=heat-bath" in the kernel note); Wolff is an error.
// grid: 0 the integer form; else 1 + k, the GRID instantiations (J on the grid 2^-k, any h: the general fp64 rule).
// tiles.S > 0 (with resident planes): the fields by rs_fields_tiles_kernel in tiles of S sites.
// run with G > 1: the replicas in row_shared_groups(a.R, G), a stream each, forked from st at the start and joined into
// it at the end (over the tile plan, without an energy trace, where row_shared_groups_fit: anything else is an error;
// " groups=G" behind the kernel note).  Null or G = 1: every launch on st, as ever.
hipError_t launch_sweep_dense_rs(const SweepArgs &a, const RowSharedPlan &p, bool j_is_i8, hipStream_t st, int grid = 0,
                                 RowSharedTiles tiles = RowSharedTiles{}, const RowSharedGroupRun *run = nullptr);

// Sequential windows (sweep_dense_seq.hip, sga_set_sequential_windows): SGA_SITE_SEQUENTIAL sweeps in windows of W
// consecutive sites -- per window one product on the matrix cores (the window-start row sums of every replica), then
// one chain wave per replica.  One dense symmetric matrix with a zero diagonal whose row sums are exact (the integer
// class, or J on the grid 2^-k).
struct SeqWindows {
    int *base = nullptr;  // [R][W] 2^k sum_j J[t0 + w][j] s_r[j] against the window-start spins (owned by the engine)
    int W = 0;            // 256 | 512 | 1024 (0: not this form)
    int grid = 0;         // 0: the integer form; else 1 + k, J on the grid 2^-k
    int mode = 0;         // the product: 0 on the int8 matrix cores (int8 rows, or the resident int8 copy j8 of fp32 rows
                          // with every |2^k J| <= 127) | 1 fp32 rows on the fp32 matrix cores
    const int8_t *j8 = nullptr;  // fp32 rows, mode 0: [n][ld8] 2^k J as int8, zero padded (made once per problem, owned by the engine)
    long long ld8 = 0;
};
inline long long seq_i8_stride(int n) { return ((long long)n + 127) / 128 * 128; }
// the resident int8 copy of fp32 rows with every |2^k J_ij| <= 127: out[i][j] = (int8)(2^k J_ij), pads zero
hipError_t launch_seq_build_i8(const float *J, long long ldj, int n, int grid_k, int8_t *out, long long ld8, hipStream_t st);
// a.n_sweeps sequential sweeps (a.site_mode == SGA_SITE_SEQUENTIAL, Philox or replayed uniforms, no per-update traces,
// all replicas): per sweep and window product + chain, then best tracking.  Any single-site rule and arithmetic: the
// decision is metropolis_accept's.  cus: compute units (the K split of the product).
hipError_t launch_sweep_dense_seq(const SweepArgs &a, const SeqWindows &sq, bool j_is_i8, int cus, hipStream_t st);

// operator-form PT exchange (cuda_kernels.py:415-443): decide sequentially, then permute rows
hipError_t launch_op_exchange(float *spins, float *tmp_rows, float *energies, const float *temps,
                              const float *u, int32_t *src_of_pos, int *n_accepted,
                              uint32_t seed_lo, uint32_t seed_hi, uint32_t round, int R, int n,
                              hipStream_t st);

// dynamic LDS bytes the dense sweep kernel needs for a given geometry
size_t sweep_dense_lds_bytes(long long ld, int table_m, bool acc64);
// integrality and max_i(sum_j |J_ij| + |h_i|) of a dense problem: out[0] = float bits of the
// max, out[1] bit 0 = some J is not an integer, bit 1 = some h is not an integer, bit 2 = some h is not a
// multiple of 1/2
hipError_t launch_dense_row_nnz(const float *J, long long ld, int n, int *nnz, hipStream_t st);  // sparse matrices given dense
hipError_t launch_dense_to_csr(const float *J, long long ld, int n, const int *rowptr, int *col, float *val, hipStream_t st);
// (n_h > 1: a shared matrix -- `rows` = n rows, each against its n_h fields h[m * rows + i]; the words of the stack)
hipError_t launch_dense_row_abs_max(const float *J, long long ldJ, const float *h, long long rows,
                                    int n, unsigned int *out, hipStream_t st, int n_h = 1);

}  // namespace sga

// (the replica measurements and moves stood here: a unit that includes this header alone still finds them)
#include "sga_replicas.h"
