// sweep_clf_fx.hip -- the cached-local-field sweep of DENSE couplings with real-valued J, as exact fixed point
// (option "clf_fixed_point").  The integer form (sweep_clf_impl.h) keeps F = scale (J s + h) as
// int16 | int32 and needs integer J; this one serves the dense problems it does not take -- half- and quarter-valued
// penalty encodings, binary-grid couplings, integer J beside an h that is no multiple of 1/2.
//
// Exactness.  The problem lies in one of the exact accumulation classes (fp32-exact: integer J, sums below 2^24;
// f64-exact: the set bits of all J and a row's carries within 53 binary places), so every row sum is exact in any order
// and the row kernels' dot is the one fp32 rounding of that exact sum.  k = minus the exponent of the lowest set bit of
// any J (0 for integer J): every 2^k J_ij is an integer, and D_i = 2^k sum_j J_ij s_j an integer below 2^53, kept EXACTLY
// in LDS as int32 | int64 (set-time scan: B = 2^k max_i sum_j |J_ij| < 2^31 | 2^62).  A proposal at site i rebuilds
// dot = fp32(2^-k D_i) -- the row kernels' dotf (sweep_dense_impl.h) -- and calls metropolis_accept on their arguments
// (h fp32, never folded into D; zero diagonal): the same decision and the same dE, E += dE in chain order.  The chain is
// the row-per-proposal chain bit for bit for every single-site rule, site mode and arithmetic.  An accept reads row i
// (fp32, or int8 for integer J) and moves D_j by -2 s_i 2^k J_ij, each entry scaled exactly in the kernel (fp64 ldexp
// -> integer), in integer arithmetic: no rounding anywhere.
//
// Mapping and windows as in sweep_clf_impl.h (its LDS layout with an empty accept table, its row chunks, its decision
// slots): one workgroup per replica (rep_list: the replicas of a mixed AUTO launch), W waves, each evaluating its own 128
// updates of a 128 W-update super-window against the state as it stands; a ballot and the slots find the earliest
// accept, all waves apply its row chunk by chunk (chunk c -> wave c mod W: no two lanes share a field, no atomics), and
// the candidates behind it are evaluated again.  The row of the PREDICTED next accept (the second accepting candidate)
// is requested while the current one is applied.  No accept table: uphill moves take the exp path of the rule.
//
// Byte model (its own, beside the graded one-row-per-proposal figure): B = acceptance x row bytes per attempt.
#include "sweep_clf_fx_impl.h"

namespace sga {

size_t sweep_clf_fx_lds_bytes(long long ldf, int field_bits, int sstride) {
    return clf_lds_bytes(ldf, field_bits / 8, sstride, 0);
}

// (fx_of and fx_apply_chunk, the exact scaling of an entry and the field update of a row chunk: sweep_clf_fx_impl.h,
//  shared with the transverse sweep on the same fields, sweep_transverse_fx.hip)

// ---- seeding: D[r][i] = 2^k sum_j J_ij s_rj, eight replicas per pass over a slice of the rows ---------------------
// Every term and partial sum is a multiple of 2^-k below 2^(53 - k) (the exact classes): the fp64 sums are exact in any
// order, and so is their scaling by 2^k.
constexpr int CLFX_SEED_REPS = 8;
template <typename JT, typename FT>
__global__ void __launch_bounds__(256) dense_fields_seed_fx_kernel(const JT *__restrict__ J, long long ldj,
                                                                   const int8_t *__restrict__ spins, int sstride, int n,
                                                                   int R, int slices, FT *__restrict__ D, long long ldf,
                                                                   int kx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned int *sb = reinterpret_cast<unsigned int *>(smem);  // [8][words]: bit = spin down
    const int words = (n + 31) / 32;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r0 = blockIdx.x * CLFX_SEED_REPS;
    for (int q = tid; q < CLFX_SEED_REPS * words; q += 256) {
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
        const JT *row = J + (long long)i * ldj;
        double acc[CLFX_SEED_REPS];
#pragma unroll
        for (int rep = 0; rep < CLFX_SEED_REPS; ++rep) acc[rep] = 0.0;
        for (int j = lane; j < n; j += 64) {
            const double x = (double)row[j];
            const int wd = j >> 5, bit = j & 31;
#pragma unroll
            for (int rep = 0; rep < CLFX_SEED_REPS; ++rep) acc[rep] += ((sb[rep * words + wd] >> bit) & 1u) ? -x : x;
        }
#pragma unroll
        for (int rep = 0; rep < CLFX_SEED_REPS; ++rep) {
            const double tot = wave_sum(acc[rep]);
            if (lane == 0 && r0 + rep < R) D[(long long)(r0 + rep) * ldf + i] = (FT)(long long)ldexp(tot, kx);
        }
    }
    // (the padding [n, ldf) of a field row: zero -- it is copied in and out of LDS and moved by the zero entries past a
    //  row's end, never read as a field)
    if (blockIdx.y == 0)
        for (int q = tid; q < CLFX_SEED_REPS * (int)(ldf - n); q += 256) {
            const int rep = q / (int)(ldf - n), i = n + q % (int)(ldf - n);
            if (r0 + rep < R) D[(long long)(r0 + rep) * ldf + i] = (FT)0;
        }
}

hipError_t launch_dense_fields_seed_fx(const void *J, bool j_is_i8, long long ldj, const int8_t *spins, int sstride, int n,
                                       int R, void *D, long long ldf, int field_bits, int k, hipStream_t st) {
    const size_t lds = (size_t)CLFX_SEED_REPS * (size_t)((n + 31) / 32) * 4;
    if (lds > 160 * 1024 || (field_bits != 32 && field_bits != 64) || ldf < n || ldj < n || (j_is_i8 && k != 0))
        return hipErrorInvalidValue;
    const int blocks = (R + CLFX_SEED_REPS - 1) / CLFX_SEED_REPS;
    const int slices = std::max(1, std::min(64, 2048 / std::max(blocks, 1)));
    auto go = [&](auto jt, auto ft) -> hipError_t {
        using JT = decltype(jt);
        using FT = decltype(ft);
        auto kern = dense_fields_seed_fx_kernel<JT, FT>;
        hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(blocks, slices), dim3(256), lds, st,
                           static_cast<const JT *>(J), ldj, spins, sstride, n, R, slices, static_cast<FT *>(D), ldf, k);
        return hipGetLastError();
    };
    if (j_is_i8) return field_bits == 64 ? go(int8_t{}, (long long)0) : go(int8_t{}, int{});
    return field_bits == 64 ? go(float{}, (long long)0) : go(float{}, int{});
}

// ---- seeding a many-model batch (sga_set_dense_batch under option "batch_fixed_point") -------------------------------
// D[r][i] = 2^k sum_j J_m[i][j] s_rj for every local replica r, m = (replica0 + r) / reps_per_model, in ONE launch whatever
// the number of models, grouped as dense_fields_seed_batch_kernel (sweep_clf.hip) groups them: a workgroup takes a GROUP
// of up to eight replicas of one model (groups never straddle a model; a shard's cut inside a group leaves the other
// side's replicas out) and a slice of that model's rows.  The sums are those of dense_fields_seed_fx_kernel: k is
// batch-wide and the class bound holds over all stacked rows, so in EVERY model each term and partial sum is a multiple
// of 2^-k below 2^(53 - k) -- fp64 sums exact in any order, and so is their scaling by 2^k.  A lane holds 16 bytes of a
// row per step (rows are padded with zeros to ldj, a multiple of 16 bytes; the spin bits past n are zero).
template <typename JT, typename FT>
__global__ void __launch_bounds__(256) dense_fields_seed_fx_batch_kernel(const JT *__restrict__ J, long long ldj, long long model_stride_j,
                                                                         const int8_t *__restrict__ spins, int sstride, int n, int R,
                                                                         unsigned int replica0, int reps_per_model, int group0,
                                                                         int slices, FT *__restrict__ D, long long ldf, int kx) {
    constexpr int EPL = 16 / (int)sizeof(JT);  // couplings per lane and step: 16 | 4
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned int *sb = reinterpret_cast<unsigned int *>(smem);  // [8][words]: bit = spin down; zero past n
    const int words = (int)((ldj + 31) / 32);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int gpm = (reps_per_model + CLFX_SEED_REPS - 1) / CLFX_SEED_REPS;  // groups per model
    const int G = group0 + (int)blockIdx.x, model = G / gpm;                // (workgroup-uniform: no divergence on the model)
    const long long g0 = (long long)model * reps_per_model + (long long)(G - model * gpm) * CLFX_SEED_REPS;  // first global replica
    const int count = (int)min((long long)CLFX_SEED_REPS, (long long)(model + 1) * reps_per_model - g0);
    // local replica of slot `rep`, -1: not in this engine's shard
    auto local = [&](int rep) -> long long {
        const long long r = g0 + rep - (long long)replica0;
        return (rep < count && r >= 0 && r < R) ? r : -1;
    };
    for (int q = tid; q < CLFX_SEED_REPS * words; q += 256) {
        const int rep = q / words, wd = q % words;
        const long long r = local(rep);
        unsigned int b = 0;
        if (r >= 0)
            for (int t = 0; t < 32; ++t) {
                const int i = 32 * wd + t;
                if (i < n && spins[r * sstride + i] < 0) b |= 1u << t;
            }
        sb[q] = b;
    }
    __syncthreads();
    const JT *Jm = J + (long long)model * model_stride_j;
    const int per = (n + slices - 1) / slices;
    const int i0 = blockIdx.y * per, i1 = min(n, i0 + per);
    using vec_t = typename std::conditional<sizeof(JT) == 4, float4, int4>::type;
    for (int i = i0 + w; i < i1; i += 4) {
        const JT *row = Jm + (long long)i * ldj;
        double acc[CLFX_SEED_REPS];
#pragma unroll
        for (int rep = 0; rep < CLFX_SEED_REPS; ++rep) acc[rep] = 0.0;
        for (long long j0 = (long long)lane * EPL; j0 < ldj; j0 += 64 * EPL) {
            const int wd = (int)(j0 >> 5), sh = (int)(j0 & 31);
            const vec_t v = *reinterpret_cast<const vec_t *>(row + j0);
            JT e[EPL];
            __builtin_memcpy(e, &v, sizeof(e));
            double x[EPL];
#pragma unroll
            for (int d = 0; d < EPL; ++d) x[d] = (double)e[d];
#pragma unroll
            for (int rep = 0; rep < CLFX_SEED_REPS; ++rep) {
                if (rep >= count) break;  // wave-uniform
                const unsigned int dn = sb[rep * words + wd] >> sh;
#pragma unroll
                for (int d = 0; d < EPL; ++d) acc[rep] += ((dn >> d) & 1u) ? -x[d] : x[d];
            }
        }
#pragma unroll
        for (int rep = 0; rep < CLFX_SEED_REPS; ++rep) {
            if (rep >= count) break;
            const double tot = wave_sum(acc[rep]);
            const long long r = local(rep);
            if (lane == 0 && r >= 0) D[r * ldf + i] = (FT)(long long)ldexp(tot, kx);
        }
    }
    // (the padding [n, ldf) of a field row: zero, as the one-model seed leaves it)
    if (blockIdx.y == 0)
        for (int q = tid; q < CLFX_SEED_REPS * (int)(ldf - n); q += 256) {
            const int rep = q / (int)(ldf - n), i = n + q % (int)(ldf - n);
            const long long r = local(rep);
            if (r >= 0) D[r * ldf + i] = (FT)0;
        }
}

hipError_t launch_dense_fields_seed_fx_batch(const void *J, bool j_is_i8, long long ldj, long long model_stride_j,
                                             const int8_t *spins, int sstride, int n, int R, unsigned int replica0,
                                             int reps_per_model, void *D, long long ldf, int field_bits, int k, hipStream_t st) {
    const size_t lds = (size_t)CLFX_SEED_REPS * (size_t)((ldj + 31) / 32) * 4;
    if (lds > 160 * 1024 || (field_bits != 32 && field_bits != 64) || ldf < n || ldj < n || sstride < n || R <= 0 ||
        reps_per_model <= 0 || (ldj * (j_is_i8 ? 1 : 4)) % 16 != 0 || (model_stride_j != 0 && model_stride_j < (long long)n * ldj) || (j_is_i8 && k != 0))  // (stride 0: one shared matrix)
        return hipErrorInvalidValue;
    // global groups [group0, group1] hold the local replicas [replica0, replica0 + R)
    const int gpm = (reps_per_model + CLFX_SEED_REPS - 1) / CLFX_SEED_REPS;
    auto group_of = [&](long long g) -> long long {
        const long long m = g / reps_per_model;
        return m * gpm + (g - m * reps_per_model) / CLFX_SEED_REPS;
    };
    const long long group0 = group_of((long long)replica0), group1 = group_of((long long)replica0 + R - 1);
    if (group1 >= (1ll << 30)) return hipErrorInvalidValue;
    const int blocks = (int)(group1 - group0 + 1);
    const int slices = std::max(1, std::min({64, 2048 / blocks, n}));
    auto go = [&](auto jt, auto ft) -> hipError_t {
        using JT = decltype(jt);
        using FT = decltype(ft);
        auto kern = dense_fields_seed_fx_batch_kernel<JT, FT>;
        hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(blocks, slices), dim3(256), lds, st, static_cast<const JT *>(J), ldj, model_stride_j, spins,
                           sstride, n, R, replica0, reps_per_model, (int)group0, slices, static_cast<FT *>(D), ldf, k);
        return hipGetLastError();
    };
    if (j_is_i8) return field_bits == 64 ? go(int8_t{}, (long long)0) : go(int8_t{}, int{});
    return field_bits == 64 ? go(float{}, (long long)0) : go(float{}, int{});
}

// ---- the sweep ------------------------------------------------------------------------------------------------
// JT: the stored row (float | int8_t), FT: the field (int | long long), BATCH: row chunks a wave requests together.
// a.field_scale = k, a.fields = D [R][ldf] FT.
// MODELS: the build for many-model batches (sga_set_dense_batch under option "batch_fixed_point"): the
// replica's model (replica0 + r) / reps_per_model is resolved once, wave-uniform, and gives the base of its rows and of
// its h -- every row base stays a scalar; offsets inside a row and a model, the LDS layout, windows, traces and best
// tracking are those of the one-model launch.  A template flag, not a run-time test: the one-model instantiations hold
// no trace of it (their code is the code they had before the flag).
template <typename JT, typename FT, int BATCH, bool MODELS>
__global__ void __launch_bounds__(64 * CLF_MAX_WAVES) sweep_clf_fx_kernel(const SweepArgs a) {
    constexpr int EPL = 16 / (int)sizeof(JT), EPC = 64 * EPL;  // elements per lane / per 1-KiB chunk
    constexpr int FB = (int)sizeof(FT);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    FT *F = reinterpret_cast<FT *>(smem);
    unsigned int *bits = reinterpret_cast<unsigned int *>(smem + clf_bits_offset(a.ldf, FB));
    // (no accept table: the decision slots follow the spin bits, where sweep_clf_impl.h's layout puts them for table_m = 0)
    int *slots2 = reinterpret_cast<int *>(smem + clf_table_offset(a.ldf, FB, a.sstride) + sizeof(float) * 4);

    const int tid = threadIdx.x, lane = tid & 63;
    const int W = (int)(blockDim.x >> 6);
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = a.rep_list ? __builtin_amdgcn_readfirstlane(a.rep_list[blockIdx.x]) : (int)blockIdx.x, n = a.n;
    const int rule = a.rule, arith = a.arith;
    const int kx = a.field_scale;  // D = 2^kx J s

    {   // resident state -> LDS
        const int4 *src = reinterpret_cast<const int4 *>(reinterpret_cast<const FT *>(a.fields) + (long long)r * a.ldf);
        int4 *dst = reinterpret_cast<int4 *>(F);
        for (int i = tid; i < (int)(a.ldf * FB / 16); i += blockDim.x) dst[i] = src[i];
        spins_to_bits(a.spins + (long long)r * a.sstride, bits, a.sstride, tid, blockDim.x);
    }
    __syncthreads();

    const JT *Jbase = reinterpret_cast<const JT *>(a.J);
    const float *hbase = a.h;
    if constexpr (MODELS) {
        const int model = __builtin_amdgcn_readfirstlane((int)((a.replica0 + (uint32_t)r) / (uint32_t)a.reps_per_model));
        Jbase += (long long)model * a.model_stride_j;
        hbase += (long long)model * n;
    }
    const int n_chunks = (int)((a.ldj + EPC - 1) / EPC);
    double E = a.energy[r], bestE = a.best_energy[r];
    unsigned long long nacc = 0;
    double T = 1.0;

    // a row is dealt to the waves in 1-KiB chunks (chunk c -> wave c mod W); a wave's first BATCH chunks are requested
    // together into registers, unconditionally (a lane past the row's end reads the row's first granule), so that the
    // request for a predicted accept can stay in flight across the next evaluation; longer rows stream the rest
    using vec_t = typename std::conditional<sizeof(JT) == 4, float4, int4>::type;
    struct RowRegs {
        vec_t x[BATCH];
    };
    auto elem0 = [&](int c) -> long long { return ((long long)c * 64 + lane) * EPL; };
    auto row_request = [&](int site) -> RowRegs {
        RowRegs o;
        const JT *row = Jbase + (long long)site * a.ldj;
#pragma unroll
        for (int q = 0; q < BATCH; ++q) {
            const long long j0 = elem0(w + q * W);
            o.x[q] = *reinterpret_cast<const vec_t *>(row + (j0 < a.ldj ? j0 : 0));
        }
        return o;
    };
    auto apply_row = [&](const RowRegs &rr, int site, int mult) {
#pragma unroll
        for (int q = 0; q < BATCH; ++q) {
            const long long j0 = elem0(w + q * W);
            if (j0 < a.ldj) fx_apply_chunk<JT, FT>(F, rr.x[q], j0, mult, kx);
        }
        const JT *row = Jbase + (long long)site * a.ldj;
        for (int c0 = w + BATCH * W; c0 < n_chunks; c0 += BATCH * W) {  // (long rows only)
            vec_t x[BATCH];
#pragma unroll
            for (int q = 0; q < BATCH; ++q) {
                const long long j0 = elem0(c0 + q * W);
                x[q] = *reinterpret_cast<const vec_t *>(row + (j0 < a.ldj ? j0 : 0));
            }
#pragma unroll
            for (int q = 0; q < BATCH; ++q) {
                const long long j0 = elem0(c0 + q * W);
                if (j0 < a.ldj) fx_apply_chunk<JT, FT>(F, x[q], j0, mult, kx);
            }
        }
    };
    auto spin_of = [&](int s) -> int { return ((bits[s >> 5] >> (s & 31)) & 1u) ? -1 : 1; };
    // the row kernels' dot: the exact sum rounded to fp32 once
    auto dot_of = [&](int s) -> float { return (float)ldexp((double)F[s], -kx); };

    int turn = 0;
    constexpr int NONE = 1 << 20;

    for (int k = 0; k < a.n_sweeps; ++k) {
        T = a.sched ? a.sched[k * a.sched_ss + r * a.sched_rs] : a.rep_temp[r];
        const long long base = (long long)r * a.replay_stride + (long long)k * n;
        for (int t0 = 0; t0 < n; t0 += CLF_WINDOW * W) {
            // this lane's two candidates: updates tA and tA + 1 of sweep k (any site mode: the general supplier)
            const int gA = w * CLF_WINDOW + 2 * lane, gB = gA + 1;  // positions in the super-window
            const int tA = t0 + gA, tB = tA + 1;
            const bool vA = tA < n, vB = tB < n;
            const UpdatePair pr = fetch_pair<false>(a, r, k, tA >> 1, vA, n);
            const int sA = pr.sA, sB = pr.sB;
            const float uA = pr.uA, uB = pr.uB;
            const float hA = hbase[sA], hB = hbase[sB];  // (static during the window)
            int pos = 0;  // super-window positions below pos are decided
            RowRegs buf0 = row_request(0), buf1 = buf0;
            int held_pos = -1;  // super-window position whose row the buffer `held` of the coming round holds (-1: none)
            auto first_of = [](unsigned long long mA, unsigned long long mB) -> int {
                const int pA = mA ? 2 * (int)__builtin_ctzll(mA) : NONE;
                const int pB = mB ? 2 * (int)__builtin_ctzll(mB) + 1 : NONE;
                return min(pA, pB);
            };
            auto round = [&](RowRegs &held, RowRegs &other) -> bool {
                int p = NONE, p2 = NONE, site = 0, site2 = 0;
                int s_old = 1;  // the spin at the first candidate's site, as evaluated
                double dE = 0.0;
                if ((w + 1) * CLF_WINDOW > pos) {  // wave-uniform (a decided window publishes "no accept")
                    const int siA = spin_of(sA), siB = spin_of(sB);
                    const float dotA = dot_of(sA), dotB = dot_of(sB);
                    double dEA = 0.0, dEB = 0.0;
                    const bool fA = (vA && gA >= pos) && metropolis_accept(rule, arith, dotA, siA, hA, 0.0f, T, uA, dEA);
                    const bool fB = (vB && gB >= pos) && metropolis_accept(rule, arith, dotB, siB, hB, 0.0f, T, uB, dEB);
                    unsigned long long mA = ballot64(fA), mB = ballot64(fB);
                    p = first_of(mA, mB);
                    if (p < NONE) {
                        if (p & 1) mB &= mB - 1;
                        else mA &= mA - 1;
                        p2 = first_of(mA, mB);
                        site = __builtin_amdgcn_readlane((p & 1) ? sB : sA, p >> 1);
                        dE = read_lane((p & 1) ? dEB : dEA, p >> 1);
                        s_old = __builtin_amdgcn_readlane((p & 1) ? siB : siA, p >> 1);
                        if (p2 < NONE) site2 = __builtin_amdgcn_readlane((p2 & 1) ? sB : sA, p2 >> 1);
                        p += w * CLF_WINDOW;
                        if (p2 < NONE) p2 += w * CLF_WINDOW;
                    }
                }
                if (W > 1) {  // the earliest window with an accept decides (sweep_clf_impl.h)
                    int *slots = slots2 + turn * (CLF_SLOT_INTS * CLF_MAX_WAVES);
                    turn ^= 1;
                    if (lane == 0) {
                        int4 *mine = reinterpret_cast<int4 *>(slots + CLF_SLOT_INTS * w);
                        const long long dbits = __double_as_longlong(dE);
                        mine[0] = make_int4(p, p2, site, site2);
                        mine[1] = make_int4((int)(unsigned int)dbits, (int)(dbits >> 32), s_old, 0);
                    }
                    __syncthreads();  // (A) every wave has evaluated against the old state and published
                    int4 q0 = make_int4(NONE, NONE, 0, 0), q1 = make_int4(0, 0, 1, 0);
                    if (lane < W) {
                        const int4 *theirs = reinterpret_cast<const int4 *>(slots + CLF_SLOT_INTS * lane);
                        q0 = theirs[0], q1 = theirs[1];
                    }
                    const unsigned long long have = ballot64(q0.x < NONE);
                    if (have == 0ull) {
                        p = NONE;
                    } else {
                        const int win = (int)__builtin_ctzll(have);
                        p = __builtin_amdgcn_readlane(q0.x, win), p2 = __builtin_amdgcn_readlane(q0.y, win);
                        site = __builtin_amdgcn_readlane(q0.z, win), site2 = __builtin_amdgcn_readlane(q0.w, win);
                        const unsigned int dlo = (unsigned int)__builtin_amdgcn_readlane(q1.x, win);
                        const unsigned int dhi = (unsigned int)__builtin_amdgcn_readlane(q1.y, win);
                        dE = __longlong_as_double((long long)(((unsigned long long)dhi << 32) | dlo));
                        s_old = __builtin_amdgcn_readlane(q1.z, win);
                        const unsigned long long later = have & (have - 1);
                        if (p2 >= NONE && later) {
                            const int nx = (int)__builtin_ctzll(later);
                            p2 = __builtin_amdgcn_readlane(q0.x, nx), site2 = __builtin_amdgcn_readlane(q0.z, nx);
                        }
                    }
                }
                if (p >= NONE) return true;  // the rest of the super-window is rejected
                if (held_pos != p) held = row_request(site);
                other = row_request(p2 < NONE ? site2 : site);
                held_pos = p2 < NONE ? p2 : -1;
                E += dE;  // (in chain order, as the row kernels add it)
                ++nacc;
                apply_row(held, site, -2 * s_old);
                if (tid == 0) {
                    bits[site >> 5] ^= 1u << (site & 31);
                    const long long upd = base + t0 + p;  // (trace buffers arrive zeroed: rejected = 0)
                    if (a.accept_trace) a.accept_trace[upd] = 1;
                    if (a.dE_trace) a.dE_trace[upd] = rule == SGA_RULE_HEAT_BATH ? -dE : dE;
                }
                pos = p + 1;
                __syncthreads();  // (B) fields and spin of the new state are visible
                return pos >= CLF_WINDOW * W;
            };
            for (;;) {
                if (round(buf0, buf1)) break;
                if (round(buf1, buf0)) break;
            }
        }
        // sweep boundary: energy record, best tracking (annealing/gpu_annealer.py:151-153)
        if (tid == 0 && a.energy_trace) a.energy_trace[(long long)k * a.R + r] = E;
        if (E < bestE && !a.no_best) {
            bestE = E;
            bits_to_spins(bits, a.best_spins + (long long)r * a.sstride, a.sstride, n, tid, blockDim.x);
        }
    }

    __syncthreads();
    {
        int4 *dst = reinterpret_cast<int4 *>(reinterpret_cast<FT *>(a.fields) + (long long)r * a.ldf);
        const int4 *src = reinterpret_cast<const int4 *>(F);
        for (int i = tid; i < (int)(a.ldf * FB / 16); i += blockDim.x) dst[i] = src[i];
        bits_to_spins(bits, a.spins + (long long)r * a.sstride, a.sstride, n, tid, blockDim.x);
    }
    if (tid == 0) {
        a.energy[r] = E;
        a.best_energy[r] = bestE;
        a.n_accepted[r] += nacc;
    }
}

// every single-site rule, site mode and arithmetic, traces included; the engine checks the problem (exact class,
// symmetric J with a zero diagonal, k, the field width)
bool sweep_clf_fx_applies(const SweepArgs &a, bool j_is_i8) {
    return a.rule != SGA_RULE_WOLFF && a.fields && (a.field_bits == 32 || a.field_bits == 64) && a.ldf >= a.ldj &&
           a.ldf % 128 == 0 && a.sstride % 32 == 0 && a.sstride >= a.n && a.table_m == 0 && !(j_is_i8 && a.field_scale != 0) &&
           a.reps_per_model >= 0 && (a.reps_per_model == 0 || a.model_stride_j == 0 || a.model_stride_j >= (long long)a.n * a.ldj) &&
           sweep_clf_fx_lds_bytes(a.ldf, a.field_bits, a.sstride) <= 160 * 1024;
}

template <typename JT, typename FT, bool MODELS>
static hipError_t launch_clf_fx(const SweepArgs &a, int waves, int n_models, hipStream_t st) {
    const size_t lds = sweep_clf_fx_lds_bytes(a.ldf, a.field_bits, a.sstride);
    const int batch = sweep_clf_batch(a.ldj, sizeof(JT) == 1, waves);
    // (int8 rows: three chunks per request -- five hold 2 x 80 bytes of row per lane and spill)
    void (*kern)(const SweepArgs) =
        (batch == 3 || sizeof(JT) == 1) ? sweep_clf_fx_kernel<JT, FT, 3, MODELS> : sweep_clf_fx_kernel<JT, FT, CLF_BATCH_MAX, MODELS>;
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(a.rep_list ? a.rep_count : a.R), dim3(64 * waves), lds, st, a);
    if constexpr (MODELS)
        note_sweep_kernel("sweep_clf_fx_kernel<%s, BATCH=%d, MODELS> x %d wave(s) (int%d fixed-point fields in LDS, k=%d, "
                          "models=%d, row read on accept only)",
                          sizeof(JT) == 4 ? "float" : "int8_t", batch, waves, a.field_bits, a.field_scale, n_models);
    else
        note_sweep_kernel("sweep_clf_fx_kernel<%s, BATCH=%d> x %d wave(s) (int%d fixed-point fields in LDS, k=%d, row read on "
                          "accept only)",
                          sizeof(JT) == 4 ? "float" : "int8_t", batch, waves, a.field_bits, a.field_scale);
    return hipGetLastError();
}

hipError_t launch_sweep_clf_fx(const SweepArgs &a, bool j_is_i8, int waves, hipStream_t st, int n_models) {
    if (waves < 1 || waves > CLF_MAX_WAVES || !sweep_clf_fx_applies(a, j_is_i8)) return hipErrorInvalidValue;
    if ((a.reps_per_model > 0) != (n_models > 1)) return hipErrorInvalidValue;
    if (a.reps_per_model > 0) {  // a many-model batch: each replica on its own model's rows
        if (j_is_i8)
            return a.field_bits == 64 ? launch_clf_fx<int8_t, long long, true>(a, waves, n_models, st)
                                      : launch_clf_fx<int8_t, int, true>(a, waves, n_models, st);
        return a.field_bits == 64 ? launch_clf_fx<float, long long, true>(a, waves, n_models, st) : launch_clf_fx<float, int, true>(a, waves, n_models, st);
    }
    if (j_is_i8)
        return a.field_bits == 64 ? launch_clf_fx<int8_t, long long, false>(a, waves, n_models, st)
                                  : launch_clf_fx<int8_t, int, false>(a, waves, n_models, st);
    return a.field_bits == 64 ? launch_clf_fx<float, long long, false>(a, waves, n_models, st) : launch_clf_fx<float, int, false>(a, waves, n_models, st);
}

}  // namespace sga
