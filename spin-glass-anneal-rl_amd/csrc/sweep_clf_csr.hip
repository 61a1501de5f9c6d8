// sweep_clf_csr.hip -- the cached-local-field sweep for SPARSE couplings (CSR): a coupling row is read only
// when a proposal is ACCEPTED (round 4; BASELINE configs[3]: the 50 000-spin scheduling instance, whose cold
// ladders reject 95 - 99 % of the proposals, and configs[1]'s assignment instance handed over sparse).
//
// Replaces the same reference code as sweep_csr_impl.h -- SpinDynamics.sweep / _metropolis_update
// (core/spin_dynamics.py:73-94,131-152) over IsingModel.get_local_field (core/ising_model.py:176-185) -- in the
// way the reference's incremental mode evaluates moves (core/energy_computer.py:166-173,262-265: dE from a
// maintained field, the field updated on a flip).  Same sites, uniforms and accept rule on exact integers: the
// chain is the row-per-proposal chain bit for bit (tests/test_cached_fields_gpu.py, against the oracle and the
// row-per-proposal CSR kernels).
//
// What is resident per replica (LDS): D_i = sum_j J_ij s_j as int16 -- the DYNAMIC part of the local field only:
// the penalty encodings' fields h_i reach 17 400 in steps of 1/2 at configs[3], far beyond 16 bits, but they
// never change; they are read (as integers scale * h_i, L2 resident) once per window with the candidates --,
// the spins as bits, the accept table.  n = 50 000: 100 KB + 6 KB + 8 KB: one replica per CU, eight waves.
// k = s_i (scale D_i + scale h_i), dE = 2 k / scale; an accept reads the row's (column, value) entries and
// moves D[column] by -2 J s_i with 16-bit LDS reads and writes (a row's columns are distinct: no two lanes
// meet; value-0 padding entries are skipped).
//
// Windows as in sweep_clf_impl.h: every wave evaluates its own 128 updates of a 128 W-update window, the waves
// meet in LDS slots, the earliest accept is applied by all, the rest is evaluated again; the entries of the
// PREDICTED next accept (the second accepting candidate) are requested together with the current row's.
//
// Byte model (its own, reported beside the graded one-row-per-proposal figure, never instead of it):
// B = acceptance rate x (deg x 8 + 8) bytes per attempt (last sentence).
//
// Fixed-point fields (option "clf_fixed_point", FX): real-valued J (acc classes f32 / f64-exact: every row sum exact)
// and integer problems whose fields outgrow int16.  k = minus the exponent of the lowest set bit of any J: every 2^k J
// is an integer, D_i = 2^k sum_j J_ij s_j an integer below 2^53, kept EXACTLY as int32 | int64.  A proposal rebuilds
// dot = fp32(2^-k D_i) -- one rounding of the exact sum, the very value the row kernels form -- and calls
// metropolis_accept on the arguments the row kernels pass (h fp32, never folded into D): the chain is theirs bit for
// bit, for every rule, site mode and arithmetic.  No accept table: uphill moves take the exp path.  An accept moves
// D[column] by -2 s_i 2^k J (the entry's fp32 value scaled in the kernel: no second copy of J) with a no-return LDS add.
//
// Ragged batches (sga_set_csr_batch under option "ragged_field_cache", RAGGED): the int16 form with one workgroup per
// replica of ANY model.  The workgroup looks its model {first row, n_m} up at entry (SweepArgs::ragged, as
// sweep_csr_impl.h) and everything that depends on the problem size uses n_m: the sites word_to_site(x, n_m), the
// window loop, the bit-to-spin write-backs (which leave the rows' padding past n_m zero).  Row extents and hq are read
// from the model's first row on; columns are model-local, so D[column] is the replica's own slice.  LDS is laid out for
// the largest model (a.ldf, a.sstride), the accept table and its scale are batch-wide: entry q stands for dE = 2 q /
// scale whatever the model, so k = s_i (scale D_i + scale h_i) decides as it would on a one-model engine.
//
// Ragged batches with fixed-point fields (options "ragged_field_cache" and "clf_fixed_point" together, RAGGED and FX):
// batches the int16 form refuses -- a model with real-valued J, an h off the half-integers, integer fields past 2^15.
// One k for the whole batch (the finest grid any model needs: every 2^k J of every model is an integer), one field
// width (int32 | int64 by 2^k max_i sum_j |J_ij| over all rows of the batch, below 2^53), h read as fp32 from the
// model's first row on.  dot = fp32(2^-k D_i) is one rounding of the exact row sum whatever k is, so each model walks
// its one-model chain.  Philox sites only; other site modes take the streaming ragged kernel.
#include "sweep_common.h"

namespace sga {

constexpr int CLFS_WINDOW = 128;     // updates a wave evaluates together: two per lane
constexpr int CLFS_MAX_WAVES = 8;
constexpr int CLFS_SLOT_INTS = 12;   // p, p2, site, site2 | k, s_old, len, len2 | beg lo, hi, beg2 lo, hi
constexpr int CLFS_SLOT_INTS_FX = 16;  // ... | dE lo, hi, -, -  (fixed-point fields)

// fb: bytes per field (2: int16, 4 | 8: fixed point)
__host__ __device__ constexpr long long clfs_bits_offset(long long ldf, int fb = 2) { return (ldf * fb + 15) & ~15ll; }
__host__ __device__ constexpr long long clfs_table_offset(long long ldf, int sstride, int fb = 2) {
    return clfs_bits_offset(ldf, fb) + (((sstride + 31) / 32 * 4 + 15) & ~15);
}
size_t sweep_clf_csr_lds_bytes(long long ldf, int sstride, int table_m, int field_bits) {
    const int fb = field_bits == 64 ? 8 : field_bits == 32 ? 4 : 2;
    return (size_t)clfs_table_offset(ldf, sstride, fb) + sizeof(float) * (size_t)((table_m + 4) & ~3) +
           2 * 4 * (fb == 2 ? CLFS_SLOT_INTS : CLFS_SLOT_INTS_FX) * CLFS_MAX_WAVES + 16;
}

// ---- seeding: D[r][i] = sum_j J_ij s_rj for eight replicas per pass over a slice of the rows -------------------
constexpr int CLFS_SEED_REPS = 8;
__global__ void __launch_bounds__(256) csr_fields_seed_kernel(const long long *__restrict__ rowptr, const int2 *__restrict__ cv,
                                                              const int8_t *__restrict__ spins, int sstride, int n, int R,
                                                              int slices, short *__restrict__ D, long long ldf) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned int *sb = reinterpret_cast<unsigned int *>(smem);  // [8][words]: bit = spin down
    const int words = (n + 31) / 32;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r0 = blockIdx.x * CLFS_SEED_REPS;
    for (int q = tid; q < CLFS_SEED_REPS * words; q += 256) {
        const int rep = q / words, wd = q % words, r = r0 + rep;
        unsigned int b = 0;
        if (r < R)
            for (int t = 0; t < 32; ++t) {
                const int i = 32 * wd + t;
                if (i < n && spins[(long long)r * sstride + i] < 0) b |= 1u << t;
            }
        sb[q] = b;
    }
    __syncthreads();
    const int per = (n + slices - 1) / slices;
    const int i0 = blockIdx.y * per, i1 = min(n, i0 + per);
    for (int i = i0 + w; i < i1; i += 4) {
        const long long beg = rowptr[i], end = rowptr[i + 1];
        int acc[CLFS_SEED_REPS];
#pragma unroll
        for (int rep = 0; rep < CLFS_SEED_REPS; ++rep) acc[rep] = 0;
        for (long long e = beg + lane; e < end; e += 64) {
            const int2 ent = cv[e];
            const int J = (int)__int_as_float(ent.y);  // integer valued (engine: eligibility)
            const int wd = ent.x >> 5, bit = ent.x & 31;
#pragma unroll
            for (int rep = 0; rep < CLFS_SEED_REPS; ++rep) acc[rep] += ((sb[rep * words + wd] >> bit) & 1u) ? -J : J;
        }
#pragma unroll
        for (int rep = 0; rep < CLFS_SEED_REPS; ++rep) {
            const int tot = wave_sum(acc[rep]);
            if (lane == 0 && r0 + rep < R) D[(long long)(r0 + rep) * ldf + i] = (short)tot;
        }
    }
}
hipError_t launch_csr_fields_seed(const long long *rowptr, const int2 *cv, const int8_t *spins, int sstride, int n, int R,
                                  short *D, long long ldf, hipStream_t st) {
    const size_t lds = (size_t)CLFS_SEED_REPS * (size_t)((n + 31) / 32) * 4;
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(csr_fields_seed_kernel), lds);
    if (e != hipSuccess) return e;
    const int blocks = (R + CLFS_SEED_REPS - 1) / CLFS_SEED_REPS;
    const int slices = std::max(1, std::min(64, 2048 / std::max(blocks, 1)));
    hipLaunchKernelGGL(csr_fields_seed_kernel, dim3(blocks, slices), dim3(256), lds, st, rowptr, cv, spins, sstride, n, R,
                       slices, D, ldf);
    return hipGetLastError();
}
// ragged batches: blockIdx.x = (model among those this engine's replicas touch, group of up to eight of ITS replicas) --
// replicas per model need not divide eight, and a shard may start inside a model: a block never straddles two models.
// FT = short: integer J summed as int (the int16 form); FT = int | long long: the fixed point D = 2^kx J s, exact fp64
// sums of integer terms below 2^53 as csr_fields_seed_fx_kernel (options "ragged_field_cache" and "clf_fixed_point").
template <typename FT>
__global__ void __launch_bounds__(256) csr_fields_seed_ragged_kernel(const long long *__restrict__ rowptr, const int2 *__restrict__ cv,
                                                                     const int8_t *__restrict__ spins, int sstride, int R,
                                                                     unsigned int replica0, int reps, int groups_per_model,
                                                                     const int2 *__restrict__ models, int slices,
                                                                     FT *__restrict__ D, long long ldf, int kx) {
    constexpr bool FX = sizeof(FT) != 2;
    using AT = std::conditional_t<FX, double, int>;  // what a term and a row sum are held in
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned int *sb = reinterpret_cast<unsigned int *>(smem);  // [8][words]: bit = spin down
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m = (int)(replica0 / (unsigned int)reps) + (int)blockIdx.x / groups_per_model;
    const int g = (int)blockIdx.x % groups_per_model;
    // the model's replicas on this engine, as local indices [lo, hi)
    const long long first = (long long)m * reps - (long long)replica0;
    const int lo = (int)max(first, 0ll) + CLFS_SEED_REPS * g, hi = (int)min(first + reps, (long long)R);
    if (lo >= hi) return;  // (block-uniform: a shard that holds part of the model)
    const int count = min(CLFS_SEED_REPS, hi - lo);
    const int2 md = models[m];
    const int n = md.y, words = (n + 31) / 32;
    rowptr += md.x;
    for (int q = tid; q < CLFS_SEED_REPS * words; q += 256) {
        const int rep = q / words, wd = q % words;
        unsigned int b = 0;
        if (rep < count)
            for (int t = 0; t < 32; ++t) {
                const int i = 32 * wd + t;
                if (i < n && spins[(long long)(lo + rep) * sstride + i] < 0) b |= 1u << t;
            }
        sb[q] = b;
    }
    __syncthreads();
    const int per = (n + slices - 1) / slices;
    const int i0 = min(n, (int)blockIdx.y * per), i1 = min(n, i0 + per);
    for (int i = i0 + w; i < i1; i += 4) {
        const long long beg = rowptr[i], end = rowptr[i + 1];
        AT acc[CLFS_SEED_REPS];
#pragma unroll
        for (int rep = 0; rep < CLFS_SEED_REPS; ++rep) acc[rep] = 0;
        for (long long e = beg + lane; e < end; e += 64) {
            const int2 ent = cv[e];
            AT J;  // an integer (engine: eligibility)
            if constexpr (FX) J = ldexp((double)__int_as_float(ent.y), kx);
            else J = (int)__int_as_float(ent.y);
            const int wd = ent.x >> 5, bit = ent.x & 31;  // (model-local column: below n)
#pragma unroll
            for (int rep = 0; rep < CLFS_SEED_REPS; ++rep) acc[rep] += ((sb[rep * words + wd] >> bit) & 1u) ? -J : J;
        }
#pragma unroll
        for (int rep = 0; rep < CLFS_SEED_REPS; ++rep) {
            const AT tot = wave_sum(acc[rep]);
            if (lane == 0 && rep < count) D[(long long)(lo + rep) * ldf + i] = FX ? (FT)(long long)tot : (FT)tot;
        }
    }
}
template <typename FT>
static hipError_t launch_seed_ragged(const long long *rowptr, const int2 *cv, const int8_t *spins, int sstride, int n_max, int R,
                                     unsigned int replica0, int reps_per_model, const int2 *models, FT *D, long long ldf, int k,
                                     hipStream_t st) {
    const size_t lds = (size_t)CLFS_SEED_REPS * (size_t)((n_max + 31) / 32) * 4;
    if (lds > 160 * 1024 || R <= 0 || reps_per_model <= 0) return hipErrorInvalidValue;
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(csr_fields_seed_ragged_kernel<FT>), lds);
    if (e != hipSuccess) return e;
    const int groups_per_model = (reps_per_model + CLFS_SEED_REPS - 1) / CLFS_SEED_REPS;
    const int n_touched = (int)((replica0 + (unsigned int)R - 1) / (unsigned int)reps_per_model - replica0 / (unsigned int)reps_per_model) + 1;
    const long long blocks = (long long)n_touched * groups_per_model;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    const int slices = (int)std::max(1ll, std::min(64ll, 2048 / blocks));
    hipLaunchKernelGGL(csr_fields_seed_ragged_kernel<FT>, dim3((unsigned int)blocks, slices), dim3(256), lds, st, rowptr, cv, spins,
                       sstride, R, replica0, reps_per_model, groups_per_model, models, slices, D, ldf, k);
    return hipGetLastError();
}
hipError_t launch_csr_fields_seed_ragged(const long long *rowptr, const int2 *cv, const int8_t *spins, int sstride, int n_max,
                                         int R, unsigned int replica0, int reps_per_model, const int2 *models, short *D,
                                         long long ldf, hipStream_t st) {
    return launch_seed_ragged<short>(rowptr, cv, spins, sstride, n_max, R, replica0, reps_per_model, models, D, ldf, 0, st);
}
hipError_t launch_csr_fields_seed_ragged_fx(const long long *rowptr, const int2 *cv, const int8_t *spins, int sstride, int n_max,
                                            int R, unsigned int replica0, int reps_per_model, const int2 *models, void *D,
                                            long long ldf, int field_bits, int k, hipStream_t st) {
    if (field_bits == 64)
        return launch_seed_ragged<long long>(rowptr, cv, spins, sstride, n_max, R, replica0, reps_per_model, models,
                                             static_cast<long long *>(D), ldf, k, st);
    if (field_bits != 32) return hipErrorInvalidValue;
    return launch_seed_ragged<int>(rowptr, cv, spins, sstride, n_max, R, replica0, reps_per_model, models, static_cast<int *>(D), ldf,
                                   k, st);
}
// fixed point: D[r][i] = 2^k sum_j J_ij s_rj as FT (int | long long).  Every term and partial sum is an integer below
// 2^53 (set-time scan): the fp64 sums are exact in any order.
template <typename FT>
__global__ void __launch_bounds__(256) csr_fields_seed_fx_kernel(const long long *__restrict__ rowptr, const int2 *__restrict__ cv,
                                                                 const int8_t *__restrict__ spins, int sstride, int n, int R,
                                                                 int slices, FT *__restrict__ D, long long ldf, int kx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned int *sb = reinterpret_cast<unsigned int *>(smem);  // [8][words]: bit = spin down
    const int words = (n + 31) / 32;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r0 = blockIdx.x * CLFS_SEED_REPS;
    for (int q = tid; q < CLFS_SEED_REPS * words; q += 256) {
        const int rep = q / words, wd = q % words, r = r0 + rep;
        unsigned int b = 0;
        if (r < R)
            for (int t = 0; t < 32; ++t) {
                const int i = 32 * wd + t;
                if (i < n && spins[(long long)r * sstride + i] < 0) b |= 1u << t;
            }
        sb[q] = b;
    }
    __syncthreads();
    const int per = (n + slices - 1) / slices;
    const int i0 = blockIdx.y * per, i1 = min(n, i0 + per);
    for (int i = i0 + w; i < i1; i += 4) {
        const long long beg = rowptr[i], end = rowptr[i + 1];
        double acc[CLFS_SEED_REPS];
#pragma unroll
        for (int rep = 0; rep < CLFS_SEED_REPS; ++rep) acc[rep] = 0.0;
        for (long long e = beg + lane; e < end; e += 64) {
            const int2 ent = cv[e];
            const double J = ldexp((double)__int_as_float(ent.y), kx);  // an integer (engine: eligibility)
            const int wd = ent.x >> 5, bit = ent.x & 31;
#pragma unroll
            for (int rep = 0; rep < CLFS_SEED_REPS; ++rep) acc[rep] += ((sb[rep * words + wd] >> bit) & 1u) ? -J : J;
        }
#pragma unroll
        for (int rep = 0; rep < CLFS_SEED_REPS; ++rep) {
            const double tot = wave_sum(acc[rep]);
            if (lane == 0 && r0 + rep < R) D[(long long)(r0 + rep) * ldf + i] = (FT)(long long)tot;
        }
    }
}
hipError_t launch_csr_fields_seed_fx(const long long *rowptr, const int2 *cv, const int8_t *spins, int sstride, int n, int R,
                                     void *D, long long ldf, int field_bits, int k, hipStream_t st) {
    const size_t lds = (size_t)CLFS_SEED_REPS * (size_t)((n + 31) / 32) * 4;
    if (lds > 160 * 1024 || (field_bits != 32 && field_bits != 64)) return hipErrorInvalidValue;
    const void *kern = field_bits == 64 ? reinterpret_cast<const void *>(csr_fields_seed_fx_kernel<long long>)
                                        : reinterpret_cast<const void *>(csr_fields_seed_fx_kernel<int>);
    hipError_t e = ensure_lds_limit(kern, lds);
    if (e != hipSuccess) return e;
    const int blocks = (R + CLFS_SEED_REPS - 1) / CLFS_SEED_REPS;
    const int slices = std::max(1, std::min(64, 2048 / std::max(blocks, 1)));
    if (field_bits == 64)
        hipLaunchKernelGGL(csr_fields_seed_fx_kernel<long long>, dim3(blocks, slices), dim3(256), lds, st, rowptr, cv, spins,
                           sstride, n, R, slices, static_cast<long long *>(D), ldf, k);
    else
        hipLaunchKernelGGL(csr_fields_seed_fx_kernel<int>, dim3(blocks, slices), dim3(256), lds, st, rowptr, cv, spins, sstride,
                           n, R, slices, static_cast<int *>(D), ldf, k);
    return hipGetLastError();
}
// hq[i] = scale * h_i as an integer (h is a multiple of 1 / scale: engine eligibility)
__global__ void scaled_fields_kernel(const float *h, int n, int scale, int *hq) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) hq[i] = (int)__builtin_rintf((float)scale * h[i]);
}
hipError_t launch_scaled_fields(const float *h, int n, int scale, int *hq, hipStream_t st) {
    hipLaunchKernelGGL(scaled_fields_kernel, dim3((n + 255) / 256), dim3(256), 0, st, h, n, scale, hq);
    return hipGetLastError();
}

// ---- the sweep ------------------------------------------------------------------------------------------------
// EPT: entries of a row per thread (the longest row <= EPT x threads of the workgroup).  FT: the field type (short;
// int | long long with FX, the fixed-point fields: a.field_scale = k, a.table_m = 0).
// RAGGED: a ragged batch -- the replica's model is looked up at entry, n is its n_m (int16, or with FX the batch-wide
// fixed point: one k and one width for every model).
template <int EPT, typename FT, bool FX, bool RAGGED = false>
__global__ void __launch_bounds__(64 * CLFS_MAX_WAVES) sweep_clf_csr_kernel(const SweepArgs a) {
    static_assert(FX == (sizeof(FT) != 2), "int16 fields: integer form; int32 | int64: fixed point");
    constexpr int SLOT_INTS = FX ? CLFS_SLOT_INTS_FX : CLFS_SLOT_INTS;
    constexpr int FB = (int)sizeof(FT);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    FT *D = reinterpret_cast<FT *>(smem);
    unsigned int *bits = reinterpret_cast<unsigned int *>(smem + clfs_bits_offset(a.ldf, FB));
    float *ptab = reinterpret_cast<float *>(smem + clfs_table_offset(a.ldf, a.sstride, FB));
    int *slots2 = reinterpret_cast<int *>(ptab + ((a.table_m + 4) & ~3));
    const int kx = FX ? a.field_scale : 0;  // D = 2^kx J s

    const int tid = threadIdx.x, lane = tid & 63;
    const int W = (int)(blockDim.x >> 6), nthreads = (int)blockDim.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = a.rep_list ? __builtin_amdgcn_readfirstlane(a.rep_list[blockIdx.x]) : (int)blockIdx.x;
    const int sc = a.table_scale;            // 1 | 2: k and the table are in units of 1 / scale
    const double inv_sc = 1.0 / (double)sc;  // exact
    const int *hq = a.clf_hq;
    const long long *rp = a.rowptr64;
    const float *hf = a.h;  // (FX: h as it is)
    // ragged batches: the replica's model {first row, spins} by its GLOBAL index (wave-uniform, scalar loads); row
    // extents and hq | h are read from the model's first row on
    int model_n = 0;
    if constexpr (RAGGED) {
        const int m = (int)((a.replica0 + (uint32_t)r) / (uint32_t)a.reps_per_model);
        const int *md = reinterpret_cast<const int *>(a.h + a.ragged) + 2 * m;
        const int model_row0 = *(const __attribute__((address_space(4))) int *)md;
        model_n = *(const __attribute__((address_space(4))) int *)(md + 1);
        if constexpr (FX) hf += model_row0;
        else hq += model_row0;
        rp += model_row0;
    }
    const int n = RAGGED ? model_n : a.n;
    // 16-byte pieces of the field slice that hold fields (ragged: the model's own n_m; what lies past is never a field)
    const int field_vecs = RAGGED ? (n * FB + 15) / 16 : (int)(a.ldf * FB / 16);
    constexpr int NONE = 1 << 30;

    {   // resident state -> LDS
        const int4 *src = reinterpret_cast<const int4 *>(reinterpret_cast<const FT *>(a.fields) + (long long)r * a.ldf);
        int4 *dst = reinterpret_cast<int4 *>(D);
        for (int i = tid; i < field_vecs; i += nthreads) dst[i] = src[i];
        const int8_t *srow = a.spins + (long long)r * a.sstride;
        spins_to_bits(srow, bits, a.sstride, tid, nthreads);
        if ((a.sstride & 31) && tid == 0) {  // (int8 layouts are padded to 16: the last half word)
            unsigned int b = 0;
            for (int t = 0; t < (a.sstride & 31); ++t) b |= (srow[(a.sstride & ~31) + t] < 0 ? 1u : 0u) << t;
            bits[a.sstride / 32] = b;
        }
    }
    __syncthreads();

    double E = a.energy[r], bestE = a.best_energy[r];
    unsigned long long nacc = 0;
    long long ksum = 0;
    double T = 1.0;
    struct RowRegs {
        int2 e[EPT];
    };
    // a row's entries, EPT per thread (entries past the row's end: column 0, value 0 -- skipped when applied)
    auto row_request = [&](long long beg, int len) -> RowRegs {
        RowRegs o;
#pragma unroll
        for (int q = 0; q < EPT; ++q) {
            const int off = tid + q * nthreads;
            o.e[q] = a.cv[beg + (off < len ? off : 0)];
            if (off >= len) o.e[q].y = 0;
        }
        return o;
    };
    auto apply_row = [&](const RowRegs &rr, int s_old) {
#pragma unroll
        for (int q = 0; q < EPT; ++q) {
            if constexpr (FX) {
                const float Jf = __int_as_float(rr.e[q].y);
                if (Jf != 0.0f) {  // 2^k J: an integer (set-time scan); the sum stays within the field's width
                    const long long d = (long long)ldexp((double)Jf, kx) * (long long)(-2 * s_old);
                    __hip_atomic_fetch_add(&D[rr.e[q].x], (FT)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            } else {
                const int J = (int)__int_as_float(rr.e[q].y);
                if (J != 0) D[rr.e[q].x] = (short)((int)D[rr.e[q].x] - 2 * J * s_old);  // (distinct columns: nobody else's)
            }
        }
    };
    int turn = 0;
    auto read_lane64 = [](long long v, int l) -> long long {
        const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)v, l);
        const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(v >> 32), l);
        return (long long)(((unsigned long long)hi << 32) | lo);
    };

    for (int k = 0; k < a.n_sweeps; ++k) {
        T = a.sched ? a.sched[k * a.sched_ss + r * a.sched_rs] : a.rep_temp[r];
        __syncthreads();
        // (entry 0 = 1 whatever T is: exp(-0 / 0) is NaN)
        for (int q = tid; q <= a.table_m; q += nthreads) ptab[q] = q == 0 ? 1.0f : expf_det((float)(-((double)(2 * q) * inv_sc) / T));
        __syncthreads();
        for (int t0 = 0; t0 < n; t0 += CLFS_WINDOW * W) {
            const int gA = w * CLFS_WINDOW + 2 * lane, gB = gA + 1;  // positions in the window
            const int tA = t0 + gA, tB = tA + 1;
            const bool vA = tA < n, vB = tB < n;
            int sA, sB;
            float uA, uB;
            if constexpr (FX) {  // any site mode: the general supplier, one pair per lane (ragged: sites of the model's n)
                const UpdatePair pr = fetch_pair<false>(a, r, k, tA >> 1, vA, n);
                sA = pr.sA, sB = pr.sB, uA = pr.uA, uB = pr.uB;
            } else {
                uint32_t key_lo = a.seed_lo, key_hi = a.seed_hi;
                asm volatile("" : "+s"(key_lo), "+s"(key_hi));
                const u32x4 x = philox4x32_10((uint32_t)(tA >> 1), a.sweep0 + (uint32_t)k, a.replica0 + (uint32_t)r, DOMAIN_SWEEP,
                                              key_lo, key_hi);
                sA = (int)word_to_site(x.x, (uint32_t)n), sB = (int)word_to_site(x.z, (uint32_t)n);
                uA = word_to_u(x.y), uB = word_to_u(x.w);
            }
            // what does not change during the window: the sites' static fields and row extents
            const int hA = FX ? 0 : hq[sA], hB = FX ? 0 : hq[sB];
            const float hfA = FX ? hf[sA] : 0.0f, hfB = FX ? hf[sB] : 0.0f;
            const long long begA = rp[sA], begB = rp[sB];
            const int lenA = (int)(rp[sA + 1] - begA), lenB = (int)(rp[sB + 1] - begB);
            int pos = 0;
            RowRegs buf0 = row_request(0, 0), buf1 = buf0;
            int held_pos = -1;
            auto first_of = [](unsigned long long mA, unsigned long long mB) -> int {
                const int pA = mA ? 2 * (int)__builtin_ctzll(mA) : NONE;
                const int pB = mB ? 2 * (int)__builtin_ctzll(mB) + 1 : NONE;
                return min(pA, pB);
            };
            auto round = [&](RowRegs &held, RowRegs &other) -> bool {
                int p = NONE, p2 = NONE, site = 0, kk = 0, s_old = 1, len = 0, len2 = 0;
                long long beg = 0, beg2 = 0;
                double dEw = 0.0;  // FX: the accepted move's dE as the rule computed it
                if ((w + 1) * CLFS_WINDOW > pos) {  // (a wave whose window is decided publishes "no accept")
                    const int siA = ((bits[sA >> 5] >> (sA & 31)) & 1u) ? -1 : 1, siB = ((bits[sB >> 5] >> (sB & 31)) & 1u) ? -1 : 1;
                    const bool liveA = vA && gA >= pos, liveB = vB && gB >= pos;
                    int kA = 0, kB = 0;
                    bool accA, accB;
                    double dEA = 0.0, dEB = 0.0;
                    if constexpr (FX) {
                        // the row kernels' dot: the exact sum rounded to fp32 once; then their accept rule on their arguments
                        // (both lanes, every proposal: no branch on the move's sign)
                        const float dotA = (float)ldexp((double)D[sA], -kx), dotB = (float)ldexp((double)D[sB], -kx);
                        accA = liveA && metropolis_accept(a.rule, a.arith, dotA, siA, hfA, 0.0f, T, uA, dEA);
                        accB = liveB && metropolis_accept(a.rule, a.arith, dotB, siB, hfB, 0.0f, T, uB, dEB);
                    } else {
                        const int fa = sc * (int)D[sA] + hA, fb = sc * (int)D[sB] + hB;
                        kA = siA * fa, kB = siB * fb;
                        accA = liveA && uA < ptab[min(max(kA, 0), a.table_m)];
                        accB = liveB && uB < ptab[min(max(kB, 0), a.table_m)];
                        const bool beyondA = liveA && kA > a.table_m, beyondB = liveB && kB > a.table_m;
                        if (ballot64(beyondA || beyondB)) {  // rare: large uphill moves (p == 0 past -104, sweep_common.h)
                            const double dA = (double)(2 * kA) * inv_sc, dB = (double)(2 * kB) * inv_sc;
                            if (beyondA) accA = !(dA > T * 104.0) && uA < expf_det((float)(-dA / T));
                            if (beyondB) accB = !(dB > T * 104.0) && uB < expf_det((float)(-dB / T));
                        }
                    }
                    unsigned long long mA = ballot64(accA), mB = ballot64(accB);
                    p = first_of(mA, mB);
                    if (p < NONE) {
                        if (p & 1) mB &= mB - 1;
                        else mA &= mA - 1;
                        p2 = first_of(mA, mB);
                        const int l1 = p >> 1;
                        site = __builtin_amdgcn_readlane((p & 1) ? sB : sA, l1);
                        if constexpr (FX) dEw = read_lane((p & 1) ? dEB : dEA, l1);
                        else kk = __builtin_amdgcn_readlane((p & 1) ? kB : kA, l1);
                        s_old = __builtin_amdgcn_readlane((p & 1) ? siB : siA, l1);
                        beg = read_lane64((p & 1) ? begB : begA, l1);
                        len = __builtin_amdgcn_readlane((p & 1) ? lenB : lenA, l1);
                        if (p2 < NONE) {
                            const int l2 = p2 >> 1;
                            beg2 = read_lane64((p2 & 1) ? begB : begA, l2);
                            len2 = __builtin_amdgcn_readlane((p2 & 1) ? lenB : lenA, l2);
                            p2 += w * CLFS_WINDOW;
                        }
                        p += w * CLFS_WINDOW;
                    }
                }
                if (W > 1) {
                    int *slots = slots2 + turn * (SLOT_INTS * CLFS_MAX_WAVES);
                    turn ^= 1;
                    if (lane == 0) {
                        int4 *mine = reinterpret_cast<int4 *>(slots + SLOT_INTS * w);
                        mine[0] = make_int4(p, p2, site, 0);
                        mine[1] = make_int4(kk, s_old, len, len2);
                        mine[2] = make_int4((int)(unsigned int)beg, (int)(beg >> 32), (int)(unsigned int)beg2, (int)(beg2 >> 32));
                        if constexpr (FX) {
                            const unsigned long long db = __builtin_bit_cast(unsigned long long, dEw);
                            mine[3] = make_int4((int)(unsigned int)db, (int)(unsigned int)(db >> 32), 0, 0);
                        }
                    }
                    __syncthreads();  // (A) every wave has evaluated against the old state and published
                    int4 q0 = make_int4(NONE, NONE, 0, 0), q1 = make_int4(0, 1, 0, 0), q2 = make_int4(0, 0, 0, 0),
                         q3 = make_int4(0, 0, 0, 0);
                    if (lane < W) {
                        const int4 *theirs = reinterpret_cast<const int4 *>(slots + SLOT_INTS * lane);
                        q0 = theirs[0], q1 = theirs[1], q2 = theirs[2];
                        if constexpr (FX) q3 = theirs[3];
                    }
                    const unsigned long long have = ballot64(q0.x < NONE);
                    if (have == 0ull) {
                        p = NONE;
                    } else {
                        const int win = (int)__builtin_ctzll(have);
                        p = __builtin_amdgcn_readlane(q0.x, win), p2 = __builtin_amdgcn_readlane(q0.y, win);
                        site = __builtin_amdgcn_readlane(q0.z, win);
                        kk = __builtin_amdgcn_readlane(q1.x, win), s_old = __builtin_amdgcn_readlane(q1.y, win);
                        len = __builtin_amdgcn_readlane(q1.z, win), len2 = __builtin_amdgcn_readlane(q1.w, win);
                        beg = (long long)(((unsigned long long)(unsigned int)__builtin_amdgcn_readlane(q2.y, win) << 32) |
                                          (unsigned int)__builtin_amdgcn_readlane(q2.x, win));
                        beg2 = (long long)(((unsigned long long)(unsigned int)__builtin_amdgcn_readlane(q2.w, win) << 32) |
                                           (unsigned int)__builtin_amdgcn_readlane(q2.z, win));
                        if constexpr (FX)
                            dEw = __builtin_bit_cast(double, ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane(q3.y, win) << 32) |
                                                                 (unsigned int)__builtin_amdgcn_readlane(q3.x, win));
                        const unsigned long long later = have & (have - 1);
                        if (p2 >= NONE && later) {  // the predicted next accept: the first of a later wave
                            const int nx = (int)__builtin_ctzll(later);
                            p2 = __builtin_amdgcn_readlane(q0.x, nx);
                            len2 = __builtin_amdgcn_readlane(q1.z, nx);
                            beg2 = (long long)(((unsigned long long)(unsigned int)__builtin_amdgcn_readlane(q2.y, nx) << 32) |
                                               (unsigned int)__builtin_amdgcn_readlane(q2.x, nx));
                        }
                    }
                }
                if (p >= NONE) return true;  // the rest of the window is rejected
                if (held_pos != p) held = row_request(beg, len);
                other = row_request(p2 < NONE ? beg2 : beg, p2 < NONE ? len2 : len);
                held_pos = p2 < NONE ? p2 : -1;
                if constexpr (FX) E += dEw;  // (in chain order, as the row kernels add it)
                else ksum += (long long)kk;
                ++nacc;
                apply_row(held, s_old);
                if (tid == 0) bits[site >> 5] ^= 1u << (site & 31);
                pos = p + 1;
                __syncthreads();  // (B) fields and spin of the new state are visible
                return pos >= CLFS_WINDOW * W;
            };
            for (;;) {
                if (round(buf0, buf1)) break;
                if (round(buf1, buf0)) break;
            }
        }
        // sweep boundary: energy record, best tracking (annealing/gpu_annealer.py:151-153)
        if constexpr (!FX) E += (double)(2 * ksum) * inv_sc;  // (integers below 2^53: exact)
        ksum = 0;
        if (tid == 0 && a.energy_trace) a.energy_trace[(long long)k * a.R + r] = E;
        if (E < bestE && !a.no_best) {
            bestE = E;
            bits_to_spins(bits, a.best_spins + (long long)r * a.sstride, a.sstride, n, tid, nthreads);
        }
    }
    __syncthreads();
    {
        int4 *dst = reinterpret_cast<int4 *>(reinterpret_cast<FT *>(a.fields) + (long long)r * a.ldf);
        const int4 *src = reinterpret_cast<const int4 *>(D);
        for (int i = tid; i < field_vecs; i += nthreads) dst[i] = src[i];
        bits_to_spins(bits, a.spins + (long long)r * a.sstride, a.sstride, n, tid, nthreads);
    }
    if (tid == 0) {
        a.energy[r] = E;
        a.best_energy[r] = bestE;
        a.n_accepted[r] += nacc;
    }
}

// production arguments only (Philox sites, Metropolis in the reference's fp64 / fp32-exp arithmetic, no per-update
// records); the engine checks the problem (integer J, sorted rows, |D| < 2^15, LDS)
// Fixed-point fields (a.field_bits = 32 | 64): every single-site rule, site mode and arithmetic; per-update records take
// the row-per-proposal kernels.
bool sweep_clf_csr_applies(const SweepArgs &a, int waves) {
    if (a.ragged && (a.rep_list || a.reps_per_model <= 0)) return false;  // ragged batches: all replicas
    // ... with fixed-point fields: Philox sites (sequential and replayed calls take the streaming ragged kernel)
    if (a.ragged && a.field_bits != 0 && (a.site_mode != SGA_SITE_RANDOM || a.replay_site || a.replay_u)) return false;
    if (a.field_bits == 32 || a.field_bits == 64)
        return !a.accept_trace && !a.dE_trace && a.rule != SGA_RULE_WOLFF && a.table_m == 0 && a.fields && a.rowptr64 &&
               a.clf_row_max <= 4 * 64 * waves && a.ldf % 8 == 0 && a.sstride % 16 == 0 &&
               sweep_clf_csr_lds_bytes(a.ldf, a.sstride, 0, a.field_bits) <= 160 * 1024;
    return a.field_bits == 0 && sweep_args_are_lean(a) && a.rule == SGA_RULE_METROPOLIS && a.table_m > 0 && a.clf_hq && a.fields &&
           a.rowptr64 && a.clf_row_max <= 4 * 64 * waves && a.ldf % 8 == 0 && a.sstride % 16 == 0 &&
           sweep_clf_csr_lds_bytes(a.ldf, a.sstride, a.table_m) <= 160 * 1024;
}

hipError_t launch_sweep_clf_csr(const SweepArgs &a, int waves, hipStream_t st) {
    if (waves < 1 || waves > CLFS_MAX_WAVES || !sweep_clf_csr_applies(a, waves)) return hipErrorInvalidValue;
    const int ept = (a.clf_row_max + 64 * waves - 1) / (64 * waves);
    void (*kern)(const SweepArgs);
    if (a.field_bits == 64 && a.ragged)
        kern = ept <= 1   ? sweep_clf_csr_kernel<1, long long, true, true>
               : ept <= 2 ? sweep_clf_csr_kernel<2, long long, true, true>
                          : sweep_clf_csr_kernel<4, long long, true, true>;
    else if (a.field_bits == 32 && a.ragged)
        kern = ept <= 1 ? sweep_clf_csr_kernel<1, int, true, true> : ept <= 2 ? sweep_clf_csr_kernel<2, int, true, true>
                                                                              : sweep_clf_csr_kernel<4, int, true, true>;
    else if (a.field_bits == 64)
        kern = ept <= 1 ? sweep_clf_csr_kernel<1, long long, true> : ept <= 2 ? sweep_clf_csr_kernel<2, long long, true>
                                                                              : sweep_clf_csr_kernel<4, long long, true>;
    else if (a.field_bits == 32)
        kern = ept <= 1 ? sweep_clf_csr_kernel<1, int, true> : ept <= 2 ? sweep_clf_csr_kernel<2, int, true>
                                                                        : sweep_clf_csr_kernel<4, int, true>;
    else if (a.ragged)
        kern = ept <= 1 ? sweep_clf_csr_kernel<1, short, false, true> : ept <= 2 ? sweep_clf_csr_kernel<2, short, false, true>
                                                                                 : sweep_clf_csr_kernel<4, short, false, true>;
    else
        kern = ept <= 1 ? sweep_clf_csr_kernel<1, short, false> : ept <= 2 ? sweep_clf_csr_kernel<2, short, false>
                                                                           : sweep_clf_csr_kernel<4, short, false>;
    const size_t lds = sweep_clf_csr_lds_bytes(a.ldf, a.sstride, a.table_m, a.field_bits);
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(a.rep_list ? a.rep_count : a.R), dim3(64 * waves), lds, st, a);
    if (a.field_bits && a.ragged)
        note_sweep_kernel("sweep_clf_csr_kernel<%d entries per thread, ragged> x %d wave(s) (int%d fixed-point fields in LDS, k=%d, "
                          "row read on accept only; each replica on its own model's rows)",
                          ept <= 1 ? 1 : ept <= 2 ? 2 : 4, waves, a.field_bits, a.field_scale);
    else if (a.field_bits)
        note_sweep_kernel("sweep_clf_csr_kernel<%d entries per thread> x %d wave(s) (int%d fixed-point fields in LDS, k=%d, "
                          "row read on accept only)",
                          ept <= 1 ? 1 : ept <= 2 ? 2 : 4, waves, a.field_bits, a.field_scale);
    else if (a.ragged)
        note_sweep_kernel("sweep_clf_csr_kernel<%d entries per thread, ragged> x %d wave(s) (int16 fields in LDS, row read on accept "
                          "only; each replica on its own model's rows)",
                          ept <= 1 ? 1 : ept <= 2 ? 2 : 4, waves);
    else
        note_sweep_kernel("sweep_clf_csr_kernel<%d entries per thread> x %d wave(s) (int16 fields in LDS, row read on accept only)",
                          ept <= 1 ? 1 : ept <= 2 ? 2 : 4, waves);
    return hipGetLastError();
}

}  // namespace sga
