// Cached-local-field sweep (sweep_clf_impl.h): instantiations and launcher.
#include "sweep_clf_impl.h"

namespace sga {

size_t sweep_clf_lds_bytes(long long ldf, int field_bits, int sstride, int table_m) {
    return clf_lds_bytes(ldf, field_bits / 8, sstride, table_m);
}

// waves per replica: enough that a wave asks for its share of a row in one batch of loads, as long as
// every replica stays resident (32 waves per CU)
int sweep_clf_waves(long long ldj, bool j_is_i8, int R, int cus, int forced /* engine option "clf_waves" */) {
    if (forced >= 1) return std::min(forced, CLF_MAX_WAVES);
    const int epc = j_is_i8 ? 1024 : 256;
    const int chunks = (int)((ldj + epc - 1) / epc);
    const int per_cu = std::max(1, (R + std::max(cus, 1) - 1) / std::max(cus, 1));
    // (the kernel holds two row buffers: ~120 VGPRs = 4 waves per SIMD = 16 resident waves per CU -- 6 or 8
    //  waves x 4 workgroups ran as two rounds of workgroups: 13.3 / 10.3 ms against 6.4 for the hot sweep)
    //  fp32 rows (4 x the chunks) measured the other way: 8 waves in two rounds 16.7 / 0.195 ms (hot / cold
    //  sweep) against 19.4 / 0.253 for 4 resident waves that stream their second batch of chunks)
    const int cap = std::max(1, std::min(CLF_MAX_WAVES, (j_is_i8 ? 16 : 32) / per_cu));
    // about three chunks per wave, from {1, 2, 3, 4, 8} (measured at 10 chunks, 1024 replicas: 1 / 2 / 3 / 4 /
    // 6 / 8 waves -> 0.28 / 0.19 / 0.175 / 0.167 / 0.173 / 0.165 ms per cold sweep, 9.3 / 6.6 / 7.2 / 7.1 /
    // 15.0 / 11.4 ms for the first, hot one: profiles/r03_experiments.md)
    const int want = (chunks + 2) / 3;  // (CLF_BATCH_MAX chunks per wave when the cap binds)
    const int pick = want <= 4 ? std::max(want, 1) : 8;
    return std::max(1, std::min(cap, pick));
}

// chunks a wave requests per row in one batch (the kernel is built for 3 and for 5)
int sweep_clf_batch(long long ldj, bool j_is_i8, int waves) {
    const int epc = j_is_i8 ? 1024 : 256;
    const int chunks = (int)((ldj + epc - 1) / epc);
    return (chunks + waves - 1) / waves <= 3 ? 3 : CLF_BATCH_MAX;
}

template <typename JT, typename FT>
static hipError_t launch_clf(const SweepArgs &a, int waves, hipStream_t st) {
    const size_t lds = clf_lds_bytes(a.ldf, (int)sizeof(FT), a.sstride, a.table_m);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const bool lean = sweep_args_are_lean(a) && a.rule == SGA_RULE_METROPOLIS;
    const int batch = sweep_clf_batch(a.ldj, sizeof(JT) == 1, waves);
    const int epc = sizeof(JT) == 1 ? 1024 : 256;
    const bool tail = (int)((a.ldj + epc - 1) / epc) > batch * waves;  // (never with 3 chunks per wave)
    void (*kern)(const SweepArgs) =
        batch == 3 ? (lean ? sweep_clf_kernel<JT, FT, true, 3, false> : sweep_clf_kernel<JT, FT, false, 3, false>)
        : tail     ? (lean ? sweep_clf_kernel<JT, FT, true, CLF_BATCH_MAX, true> : sweep_clf_kernel<JT, FT, false, CLF_BATCH_MAX, true>)
                   : (lean ? sweep_clf_kernel<JT, FT, true, CLF_BATCH_MAX, false>
                           : sweep_clf_kernel<JT, FT, false, CLF_BATCH_MAX, false>);
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(a.rep_list ? a.rep_count : a.R), dim3(64 * waves), lds, st, a);
    note_sweep_kernel("sweep_clf_kernel<%s, %s, %s, BATCH=%d, TAIL=%d> x %d wave(s)", sizeof(JT) == 4 ? "float" : "int8_t",
                      sizeof(FT) == 2 ? "int16_t" : "int32_t", lean ? "LEAN" : "general", batch, (int)tail, waves);
    return hipGetLastError();
}

// ---- seeding the fields of a many-model batch (sga_set_dense_batch) ---------------------------------------------------
// F[r][i] = scale (sum_j J_m[i][j] s_rj + h_m[i]) for every local replica r, m = (replica0 + r) / reps_per_model, in ONE
// launch whatever the number of models: a workgroup takes a GROUP of up to eight replicas of one model (groups never
// straddle a model; a shard's cut inside a group leaves the other side's replicas out) and a slice of the model's rows.
// The spins live in LDS as bits (1 = down); a lane holds 16 bytes of a row and adds, per replica, the couplings under the
// down bits:  J s = sum_j J_ij - 2 sum_{j down} J_ij.  int8 rows: 4 bits -> a byte mask (one multiply, two ands, one
// multiply), v_dot4_i32_i8 against 0x01010101 sums the selected bytes -- 1.5 VALU instructions per coupling and replica;
// fp32 rows (integer valued, |sums| < 2^24): converted once, added under the bit.  Everything is an integer below 2^24:
// int32 sums in any order are exact, the fields carry the bits the one-model matrix-core pass (fields_dense.hip) gives.
// Why not that pass with a model coordinate: its tile is 128 replicas, a batch has 1 ... 8 per model as a rule (a tile
// >= 94 % empty, its Y scratch and finish pass on top); here a model with k replicas is read ceil(k / 8) times -- once
// for k <= 8, the bytes of the whole stack once -- and nothing but the fields is written.
constexpr int CLF_SEED_REPS = 8;
template <typename JT, typename FT>
__global__ void __launch_bounds__(256) dense_fields_seed_batch_kernel(const JT *__restrict__ J, long long ldj, long long model_stride_j,
                                                                      const float *__restrict__ h, const int8_t *__restrict__ spins,
                                                                      int sstride, int n, int R, unsigned int replica0,
                                                                      int reps_per_model, int group0, int slices,
                                                                      FT *__restrict__ F, long long ldf, int scale) {
    constexpr int EPL = 16 / (int)sizeof(JT);  // couplings per lane and step: 16 | 4
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned int *sb = reinterpret_cast<unsigned int *>(smem);  // [8][words]: bit = spin down; zero past n
    const int words = (int)((ldj + 31) / 32);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int gpm = (reps_per_model + CLF_SEED_REPS - 1) / CLF_SEED_REPS;  // groups per model
    const int G = group0 + (int)blockIdx.x, model = G / gpm;
    const long long g0 = (long long)model * reps_per_model + (long long)(G - model * gpm) * CLF_SEED_REPS;  // first global replica
    const int count = (int)min((long long)CLF_SEED_REPS, (long long)(model + 1) * reps_per_model - g0);
    // local replica of slot `rep`, -1: not in this engine's shard
    auto local = [&](int rep) -> long long {
        const long long r = g0 + rep - (long long)replica0;
        return (rep < count && r >= 0 && r < R) ? r : -1;
    };
    for (int q = tid; q < CLF_SEED_REPS * words; q += 256) {
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
    const float *hm = h + (long long)model * n;
    const int per = (n + slices - 1) / slices;
    const int i0 = blockIdx.y * per, i1 = min(n, i0 + per);
    for (int i = i0 + w; i < i1; i += 4) {
        const JT *row = Jm + (long long)i * ldj;
        int tot = 0, down[CLF_SEED_REPS];
#pragma unroll
        for (int rep = 0; rep < CLF_SEED_REPS; ++rep) down[rep] = 0;
        // (a row is padded with zeros to ldj, a multiple of 128 bytes: every 16-byte step below ldj lies inside it)
        for (long long j0 = (long long)lane * EPL; j0 < ldj; j0 += 64 * EPL) {
            const int wd = (int)(j0 >> 5), sh = (int)(j0 & 31);
            if constexpr (sizeof(JT) == 1) {
                const int4 x = *reinterpret_cast<const int4 *>(row + j0);
                const int xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int d = 0; d < 4; ++d) tot = __builtin_amdgcn_sdot4(xs[d], 0x01010101, tot, false);
#pragma unroll
                for (int rep = 0; rep < CLF_SEED_REPS; ++rep) {
                    if (rep >= count) break;  // wave-uniform
                    const unsigned int hw = (sb[rep * words + wd] >> sh) & 0xFFFFu;
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const unsigned int nib = (hw >> (4 * d)) & 15u;
                        const unsigned int mask = ((nib * 0x00204081u) & 0x01010101u) * 0xFFu;  // bit b -> byte b
                        down[rep] = __builtin_amdgcn_sdot4(xs[d] & (int)mask, 0x01010101, down[rep], false);
                    }
                }
            } else {
                const float4 x = *reinterpret_cast<const float4 *>(row + j0);
                const int xs[4] = {(int)x.x, (int)x.y, (int)x.z, (int)x.w};  // integer valued below 2^24: exact
                tot += (xs[0] + xs[1]) + (xs[2] + xs[3]);
#pragma unroll
                for (int rep = 0; rep < CLF_SEED_REPS; ++rep) {
                    if (rep >= count) break;  // wave-uniform
                    const unsigned int nib = (sb[rep * words + wd] >> sh) & 15u;
#pragma unroll
                    for (int d = 0; d < 4; ++d) down[rep] += xs[d] & -(int)((nib >> d) & 1u);
                }
            }
        }
        tot = wave_sum(tot);
        const int hq = (int)((float)scale * hm[i]);  // h is a multiple of 1 / scale: exact
#pragma unroll
        for (int rep = 0; rep < CLF_SEED_REPS; ++rep) {
            if (rep >= count) break;
            const int dn = wave_sum(down[rep]);
            const long long r = local(rep);
            if (lane == 0 && r >= 0) F[r * ldf + i] = (FT)(scale * (tot - 2 * dn) + hq);
        }
    }
    // (the padding [n, ldf) of a field row: zero -- copied in and out of LDS, moved by the zero entries past a row's end,
    //  never read as a field)
    if (blockIdx.y == 0)
        for (int q = tid; q < CLF_SEED_REPS * (int)(ldf - n); q += 256) {
            const int rep = q / (int)(ldf - n), i = n + q % (int)(ldf - n);
            const long long r = local(rep);
            if (r >= 0) F[r * ldf + i] = (FT)0;
        }
}

hipError_t launch_dense_fields_seed_batch(const void *J, bool j_is_i8, long long ldj, long long model_stride_j, const float *h,
                                          const int8_t *spins, int sstride, int n, int R, unsigned int replica0,
                                          int reps_per_model, void *F, long long ldf, int field_bits, int scale,
                                          hipStream_t st) {
    const size_t lds = (size_t)CLF_SEED_REPS * (size_t)((ldj + 31) / 32) * 4;
    if (lds > 160 * 1024 || (field_bits != 16 && field_bits != 32) || ldf < n || ldj < n || sstride < n || R <= 0 ||
        reps_per_model <= 0 || (ldj * (j_is_i8 ? 1 : 4)) % 16 != 0 || (scale != 1 && scale != 2))
        return hipErrorInvalidValue;
    // global groups [group0, group1] hold the local replicas [replica0, replica0 + R)
    const int gpm = (reps_per_model + CLF_SEED_REPS - 1) / CLF_SEED_REPS;
    auto group_of = [&](long long g) -> long long {
        const long long m = g / reps_per_model;
        return m * gpm + (g - m * reps_per_model) / CLF_SEED_REPS;
    };
    const long long group0 = group_of((long long)replica0), group1 = group_of((long long)replica0 + R - 1);
    if (group1 >= (1ll << 30)) return hipErrorInvalidValue;
    const int blocks = (int)(group1 - group0 + 1);
    const int slices = std::max(1, std::min({64, 2048 / blocks, n}));
    auto go = [&](auto jt, auto ft) -> hipError_t {
        using JT = decltype(jt);
        using FT = decltype(ft);
        auto kern = dense_fields_seed_batch_kernel<JT, FT>;
        hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(blocks, slices), dim3(256), lds, st, static_cast<const JT *>(J), ldj, model_stride_j, h,
                           spins, sstride, n, R, replica0, reps_per_model, (int)group0, slices, static_cast<FT *>(F), ldf, scale);
        return hipGetLastError();
    };
    if (j_is_i8) return field_bits == 16 ? go(int8_t{}, int16_t{}) : go(int8_t{}, int32_t{});
    return field_bits == 16 ? go(float{}, int16_t{}) : go(float{}, int32_t{});
}

hipError_t launch_sweep_clf(const SweepArgs &a, bool j_is_i8, int waves, hipStream_t st) {
    if (waves < 1 || waves > CLF_MAX_WAVES || !a.fields || (a.field_bits != 16 && a.field_bits != 32) ||
        (a.ldf * (a.field_bits / 8)) % 16 != 0 || a.sstride % 32 != 0)
        return hipErrorInvalidValue;
    if (j_is_i8)
        return a.field_bits == 16 ? launch_clf<int8_t, int16_t>(a, waves, st) : launch_clf<int8_t, int32_t>(a, waves, st);
    return a.field_bits == 16 ? launch_clf<float, int16_t>(a, waves, st) : launch_clf<float, int32_t>(a, waves, st);
}

}  // namespace sga
