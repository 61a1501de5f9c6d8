// worldline_clusters_dense.hip -- world-line cluster updates on DENSE couplings, decided on the cached local fields
// (sga_worldline_clusters_dense).
//
// The step is sga_worldline_clusters' (worldline_clusters.hip): groups, typewriter order, one Philox block per slice and
// site, segments from the bonds, the fp64 Metropolis rule on the head's lane.  The row sum comes from the resident fields
// F = scale (J s + h) of every slice, dot_p = (F_p[i] - scale h_i) / scale -- the identity sweep_transverse_clf.hip decides
// on -- so a coupling row is read only for a site where a segment flips, and the fields are kept valid for every flip.
//
// One launch per call, one workgroup of W waves per group.  A group's fields (P ldf elements) stay in HBM / L2; only this
// workgroup touches them during the launch, __syncthreads() orders one wave's global stores before another wave's loads.
// The sites go in BLOCKS of B consecutive sites, each block in two phases:
//   A, decide (wave 0, lane p = slice p): the block's B fields of the lane's slice in registers as int32, its B int8 spins
//      in registers; the B x B tile of J, h_i and scale h_i staged in LDS by all waves before.  Per site the draw, a ballot
//      of the signs, a ballot of the bonds, heads and sizes by clz / ctz, the segment sums through LDS integer atomics (as
//      in worldline_clusters.hip), the rule, a ballot of the flipped lanes.  A flipped lane negates its spin byte, moves its
//      energy and corrects its registers of the later sites of the block from the tile (a broadcast read).  (flip mask,
//      sign mask) of every site go to a list in LDS.  No global access between the first and the last site of a block.
//   B, apply (all waves, after a barrier): for every listed site with a flip, row i of J is dealt to the waves in 1-KiB
//      chunks, chunk c -> wave c mod W, and F_p[j] -= 2 scale sigma_p J_ij for every flipped slice p, 16-byte global loads
//      and stores, packed int16 where the fields are int16 (clf_fields_update) -- the block's own columns included.
// A lane past the row's end loads at a clamped index and stores nothing: no load under a lane condition.  No scratch.
#include "sga_quantum.h"
#include "sweep_clf_impl.h"

namespace sga {

namespace {

#ifndef SGA_WLD_BLOCK
#define SGA_WLD_BLOCK 32  // (-DSGA_WLD_BLOCK=16 | 64: the builds DESIGN.md 4.12 measured beside this one)
#endif
constexpr int WLD_BLOCK = SGA_WLD_BLOCK;  // B: sites decided between two applications of rows
static_assert(WLD_BLOCK == 16 || WLD_BLOCK == 32 || WLD_BLOCK == 64, "a block is 16, 32 or 64 sites");

template <typename JT, typename FT, int B>
__global__ void __launch_bounds__(64 * CLF_MAX_WAVES) worldline_clusters_dense_kernel(const SweepArgs a, const WorldlineArgs q) {
    constexpr int EPL = 16 / (int)sizeof(JT), EPC = 64 * EPL;  // elements per lane / per 1-KiB chunk
    constexpr int FB = (int)sizeof(FT);
    constexpr int FV = B * FB / 16, SV = B / 16;  // int4 of a lane's fields / spins of a block
    using vec_t = typename std::conditional<sizeof(JT) == 4, float4, int4>::type;
    __shared__ __attribute__((aligned(16))) int tile[B][B];  // J[b0 + k][b0 + k2]
    __shared__ float h_blk[B];
    __shared__ int hq_blk[B];                                 // scale h_i
    __shared__ int acc[64];
    __shared__ unsigned long long flip_list[B], sign_list[B];
    __shared__ unsigned long long best_mask;

    const int tid = threadIdx.x, lane = tid & 63;
    const int W = (int)(blockDim.x >> 6);
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = (int)blockIdx.x;
    const int P = q.n_slices, n = a.n;
    const int G = a.R / P;
    const int sc = a.field_scale, sh = sc >> 1;  // scale 1 | 2: the division is a shift by 0 | 1
    const bool mine = lane < P;
    const int p = mine ? lane : P - 1;  // lanes >= P run along on slice P - 1 and store nothing
    const int r = slice_row(g, P, p);
    const int pn = ring_next(p, P);
    const unsigned long long ring = P == 64 ? ~0ull : (1ull << P) - 1ull;
    const JT *Jbase = reinterpret_cast<const JT *>(a.J);
    FT *Fgroup = reinterpret_cast<FT *>(a.fields) + (long long)slice_row(g, P, 0) * a.ldf;
    FT *Fmine = reinterpret_cast<FT *>(a.fields) + (long long)r * a.ldf;
    int8_t *smine = a.spins + (long long)r * a.sstride;
    const int n_chunks = (int)((a.ldj + EPC - 1) / EPC);

    const double T = a.rep_temp[g * P];
    double E = a.energy[r], bestE = a.best_energy[r];  // (wave 0's are the ones kept)
    long long n_seg = 0, n_segflip = 0, n_spinflip = 0;
    if (tid < 64) acc[tid] = 0;

    for (int kk = 0; kk < q.n_sweeps; ++kk) {
        const uint32_t thr = q.thr[(size_t)kk * G + g];
        for (int b0 = 0; b0 < n; b0 += B) {
            const int nb = n - b0 < B ? n - b0 : B;  // the tail block is shorter
            // ---- all waves: the block's tile of J, h and scale h into LDS (rows and columns clamped into the matrix)
            for (int t = tid; t < B * B; t += (int)blockDim.x) {
                const int k = t / B, k2 = t % B;
                const int row = b0 + k < n ? b0 + k : n - 1;
                const long long col = b0 + k2 < a.ldj ? b0 + k2 : a.ldj - 1;
                tile[k][k2] = (int)Jbase[(long long)row * a.ldj + col];
            }
            if (tid < B) {
                const float h = a.h[b0 + tid < n ? b0 + tid : n - 1];
                h_blk[tid] = h;
                hq_blk[tid] = (int)((float)sc * h);  // h is a multiple of 1 / scale: exact
            }
            __syncthreads();  // (1) the tile stands; the fields of phase B before it are visible

            // ---- phase A: wave 0 decides the block's sites
            if (w == 0) {
                int Fr[B];
                uint32_t sp[B / 4];
                {
                    const int4 *fsrc = reinterpret_cast<const int4 *>(Fmine + b0);
#pragma unroll
                    for (int v = 0; v < FV; ++v) {
                        const int4 x = fsrc[v];
                        const int d[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            if constexpr (FB == 2) {
                                Fr[8 * v + 2 * c] = (int)(short)(d[c] & 0xFFFF);
                                Fr[8 * v + 2 * c + 1] = d[c] >> 16;
                            } else {
                                Fr[4 * v + c] = d[c];
                            }
                        }
                    }
                    const int4 *ssrc = reinterpret_cast<const int4 *>(smine + b0);
#pragma unroll
                    for (int v = 0; v < SV; ++v) {
                        const int4 x = ssrc[v];
                        sp[4 * v] = (uint32_t)x.x, sp[4 * v + 1] = (uint32_t)x.y, sp[4 * v + 2] = (uint32_t)x.z, sp[4 * v + 3] = (uint32_t)x.w;
                    }
                }
#pragma unroll
                for (int k = 0; k < B; ++k) {
                    if (k >= nb) continue;  // wave-uniform: the tail block
                    const int i = b0 + k;
                    const u32x4 rnd = worldline_block((uint32_t)i, q.round + (uint32_t)kk, a.replica0 + (uint32_t)r, a.seed_lo, a.seed_hi);
                    const float h = h_blk[k];
                    const int dot = (Fr[k] - hq_blk[k]) >> sh;  // (F - scale h is scale times an integer: the shift is exact)
                    // signs, bonds, heads, segments
                    const uint32_t sb = (sp[k >> 2] >> (8 * (k & 3) + 7)) & 1u;
                    const unsigned long long word = ballot64(mine && sb != 0u);  // bit p = [s_p[i] < 0]
                    const bool bond = mine && sb == ((uint32_t)(word >> pn) & 1u) && (rnd.x >> 8) < thr;
                    const unsigned long long bonds = ballot64(bond);
                    unsigned long long heads = ~((bonds << 1) | (bonds >> (P - 1))) & ring;  // head iff the bond below is open
                    if (heads == 0) heads = 1ull;  // no head: the whole ring, head 0
                    const unsigned long long below = heads & ((2ull << p) - 1ull);  // (p = 63: 2 << 63 = 0, the mask all ones)
                    const int f = 63 - __builtin_clzll(below ? below : heads);       // the wrap through slice 0
                    const unsigned long long above = heads & ~((2ull << p) - 1ull);
                    const int next_head = __builtin_ctzll(above ? above : heads);
                    const int m = above ? next_head - p : P - p + next_head;  // the size of a segment whose head is p
                    atomicAdd(&acc[f], mine ? dot : 0);
                    __builtin_amdgcn_wave_barrier();
                    const int A = atomicExch(&acc[lane], 0);
                    __builtin_amdgcn_wave_barrier();
                    // the decision, on the head's lane (the other lanes compute along and are not looked at)
                    const double sigma = sb ? -1.0 : 1.0;
                    const double Phi = (double)A + (double)m * (double)h;
                    const double dE = 2.0 * sigma * Phi;
                    bool flip = dE <= 0.0;
                    if (!flip && !(dE > T * 104.0))  // (beyond: the fp32 argument is below expf_det's underflow bound, p = 0)
                        flip = (double)word_to_u(rnd.y) < (double)expf_det((float)(-dE / T));
                    const bool is_head = mine && ((heads >> p) & 1ull);
                    const unsigned long long flipped_heads = ballot64(is_head && flip);
                    const bool my_flip = mine && ((flipped_heads >> f) & 1ull);
                    const unsigned long long flips = ballot64(my_flip);
                    if (my_flip) {
                        sp[k >> 2] ^= 0xFEu << (8 * (k & 3));  // +1 (0x01) <-> -1 (0xFF)
                        E += 2.0 * sigma * ((double)dot + (double)h);
                    }
                    if (flips != 0ull) {  // wave-uniform: the lane's fields of the later sites of the block
                        const int mult = my_flip ? (sb ? 2 * sc : -2 * sc) : 0;  // -2 scale sigma
#pragma unroll
                        for (int k2 = k + 1; k2 < B; ++k2) Fr[k2] += mult * tile[k][k2];
                    }
                    if (lane == 0) flip_list[k] = flips, sign_list[k] = word;
                    n_seg += __builtin_popcountll(heads);
                    n_segflip += __builtin_popcountll(flipped_heads);
                    n_spinflip += __builtin_popcountll(flips);
                }
                if (mine) {
                    int4 *sdst = reinterpret_cast<int4 *>(smine + b0);
#pragma unroll
                    for (int v = 0; v < SV; ++v) sdst[v] = make_int4((int)sp[4 * v], (int)sp[4 * v + 1], (int)sp[4 * v + 2], (int)sp[4 * v + 3]);
                }
            }
            __syncthreads();  // (2) the list stands

            // ---- phase B: all waves apply the flipped sites' rows to the flipped slices' fields
            for (int k = 0; k < nb; ++k) {
                const unsigned long long fl = flip_list[k];
                const uint32_t flo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)fl);
                const uint32_t fhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(fl >> 32));
                unsigned long long flips = ((unsigned long long)fhi << 32) | flo;
                if (flips == 0ull) continue;  // wave-uniform
                const unsigned long long sg = sign_list[k];
                const uint32_t slo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)sg);
                const uint32_t shi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(sg >> 32));
                const unsigned long long signs = ((unsigned long long)shi << 32) | slo;
                const JT *row = Jbase + (long long)(b0 + k) * a.ldj;
                for (int c = w; c < n_chunks; c += W) {
                    const long long j0 = ((long long)c * 64 + lane) * EPL;
                    const bool inside = j0 < a.ldj;
                    const long long jc = inside ? j0 : 0;  // (a clamped index: the load stands under no condition)
                    const vec_t x = *reinterpret_cast<const vec_t *>(row + jc);
                    for (unsigned long long todo = flips; todo; todo &= todo - 1) {
                        const int pp = __builtin_ctzll(todo);
                        FT *F = Fgroup + (long long)pp * a.ldf;
                        ClfFields<JT, FT> fv = clf_fields_load<JT, FT>(F, jc);
                        if ((signs >> pp) & 1ull)  // sigma = -1: mult = +2 scale
                            clf_fields_update<JT, FT, false>(fv, x, 2 * sc, sc);
                        else
                            clf_fields_update<JT, FT, true>(fv, x, -2 * sc, sc);
                        if (inside) clf_fields_store<JT, FT>(F, j0, fv);
                    }
                }
            }
            // (the next block's barrier (1) orders these stores before its loads, and the list's readers before its writer)
        }
        // ---- the sweep's end: the best follows where the energy is lower
        if (w == 0) {
            const bool lower = mine && E < bestE;
            if (lower) bestE = E;
            const unsigned long long todo = ballot64(lower);
            if (lane == 0) best_mask = todo;
        }
        __syncthreads();  // (3) the mask stands, the spins of the last block are visible
        {
            const unsigned long long bm = best_mask;
            const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bm);
            const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bm >> 32));
            for (unsigned long long todo = ((unsigned long long)bhi << 32) | blo; todo; todo &= todo - 1) {
                const int pp = __builtin_ctzll(todo);
                const int4 *src = reinterpret_cast<const int4 *>(a.spins + (long long)slice_row(g, P, pp) * a.sstride);
                int4 *dst = reinterpret_cast<int4 *>(a.best_spins + (long long)slice_row(g, P, pp) * a.sstride);
                for (int c = tid; c < a.sstride / 16; c += (int)blockDim.x) dst[c] = src[c];
            }
        }
        __syncthreads();  // (4) the rows are copied before the next sweep writes spins, the mask read before it is written
    }

    if (w == 0) {
        if (mine) {
            a.energy[r] = E;
            a.best_energy[r] = bestE;
        }
        if (q.stats && lane < 3) q.stats[3 * g + lane] = lane == 0 ? n_seg : lane == 1 ? n_segflip : n_spinflip;
    }
}

template <typename JT, typename FT>
hipError_t launch_wld(const SweepArgs &a, const WorldlineArgs &w, int waves, hipStream_t st) {
    constexpr int B = WLD_BLOCK;
    hipLaunchKernelGGL((worldline_clusters_dense_kernel<JT, FT, B>), dim3(a.R / w.n_slices), dim3(64 * waves), 0, st, a, w);
    note_sweep_kernel("worldline_clusters_dense_kernel<%s, %s, B=%d, %d slices> x %d sweep(s) x %d wave(s)", sizeof(JT) == 4 ? "float" : "int8_t",
                      sizeof(FT) == 2 ? "int16_t" : "int32_t", B, w.n_slices, w.n_sweeps, waves);
    return hipGetLastError();
}

}  // namespace

int worldline_dense_waves(long long ldj, bool j_is_i8, int forced /* engine option "clf_waves" */) {
    if (forced >= 1) return forced < CLF_MAX_WAVES ? forced : CLF_MAX_WAVES;
    // G workgroups on G compute units: as many waves as a row has 1-KiB chunks, up to the eight of a workgroup
    const long long epc = j_is_i8 ? 1024 : 256;
    const long long chunks = (ldj + epc - 1) / epc;
    return chunks < 1 ? 1 : chunks > CLF_MAX_WAVES ? CLF_MAX_WAVES : (int)chunks;
}

hipError_t launch_worldline_clusters_dense(const SweepArgs &a, const WorldlineArgs &w, bool j_is_i8, int waves, hipStream_t st) {
    if (waves < 1 || waves > CLF_MAX_WAVES || !a.J || !a.h || !a.spins || !a.best_spins || !a.energy || !a.best_energy ||
        !a.rep_temp || !a.fields || !w.thr || (a.field_bits != 16 && a.field_bits != 32) || (a.field_scale != 1 && a.field_scale != 2) ||
        (a.ldf * (a.field_bits / 8)) % 16 != 0 || a.ldf % WLD_BLOCK != 0 || a.sstride % WLD_BLOCK != 0 || a.sstride % 16 != 0 || a.sstride < a.n || a.ldf < a.ldj || a.ldj < a.n ||
        (a.ldj * (j_is_i8 ? 1 : 4)) % 16 != 0 || a.n < 1 || w.n_slices < 2 || w.n_slices > WORLDLINE_MAX_SLICES || a.R % w.n_slices != 0 ||
        a.replica0 % (uint32_t)w.n_slices != 0 || w.n_sweeps < 1)
        return hipErrorInvalidValue;
    if (j_is_i8) return a.field_bits == 16 ? launch_wld<int8_t, int16_t>(a, w, waves, st) : launch_wld<int8_t, int32_t>(a, w, waves, st);
    return a.field_bits == 16 ? launch_wld<float, int16_t>(a, w, waves, st) : launch_wld<float, int32_t>(a, w, waves, st);
}

}  // namespace sga
