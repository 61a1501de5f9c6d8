// sweep_dense_seq.hip -- "sequential windows": SGA_SITE_SEQUENTIAL sweeps of many replicas with ONE read of each
// coupling row per sweep (sga_set_sequential_windows).
//
// In the typewriter order of the reference's GPU path (annealing/cuda_kernels.py:381) update t of a sweep proposes site
// t in every replica.  A sweep is cut into windows of W consecutive updates t0 ... t0 + W - 1; each window runs
//   * product: base[r][w] = 2^k sum_j J[t0 + w][j] s_r[j] against the window-start spins of ALL replicas, a
//     (W x n) . (n x R) product on the matrix cores.  Both operands are read straight from their row-major rows (a spin
//     row, a coupling row: 16 contiguous bytes per lane and K step, the layout of fields_mfma_kernel), the K range is
//     split over workgroups and the partial sums meet in integer atomics;
//   * chain: one wave per replica holds the W pending fields, one per (lane, block of 64 updates), and walks the blocks
//     in order.  A block first takes the corrections -2 J[i_a][t] s_a (J symmetric: read from row i_a, contiguous
//     across the lanes) of every accept the window has made so far; then its 64 updates are decided at once, the
//     couplings of the first few accepting ones to the block are fetched together and accepts are committed in chain
//     order from registers (the block logic of rs_chain_kernel, sweep_dense_rs.hip).  No site repeats inside a window,
//     so there are no spin bit-planes, no plan and no repeat-site negation.
//
// The problems (sga_engine.cpp, sequential_windows): J symmetric with a zero diagonal, and either the integer class
// (k = 0: J and h integer valued, max_i (sum_j |J_ij| + |h_i|) < 2^24) or the set-time grid verdict of option
// "row_shared_grid" (every J_ij an integer multiple of 2^-k, k <= 30, B = 2^k max_i sum_j |J_ij| < 2^24, any finite h).
//
// Exactness of the product.  Write m_ij = 2^k J_ij, an integer, and s_j = +-1.
//   * int8 matrix cores (int8 rows, and fp32 rows with every |m_ij| <= 127 through a resident int8 copy made once per
//     problem, as the row-shared windows' bit-planes are -- seq_to_i8_kernel: m_ij = (int)(J_ij 2^k),
//     a power-of-two multiply of a value on the grid and a conversion of an integer, both exact; |m_ij| <= 127 fits
//     int8): products and sums are int32 arithmetic with |any partial sum| <= sum_j |m_ij| <= B < 2^24 -- no overflow,
//     no rounding, in any order.
//   * fp32 matrix cores (other fp32 rows): a product J_ij s_j is +-J_ij, exact.  Any partial sum of a row, over any
//     subset of the columns in any order, is 2^-k times an integer of magnitude at most B < 2^24, hence representable in
//     fp32 (24 significant bits, and the exponent stays in range: k <= 30), so every fma of the k-ordered chain inside
//     the matrix core returns the exact sum.  The result D = (int)(acc 2^k) is again an exact scaling and conversion.
//   * K split: a workgroup's partial sum over its K range is one of those partial sums (exact), and the int32
//     atomicAdd of partial integers is associative: base is the exact D whatever the split and the order of arrival.
//     Zero-padded columns (J rows are zero padded to their stride, spin pads are 0) add exact zeros.
// So base[r][w] = D exactly, and f = ldexpf((float)D, -k) is the exact row sum (|D| < 2^24).
//
// Exactness of the chain.  A correction -2 J[i_a][t] s_a is an integer multiple of 2^-k (the fp32 J itself, or the int8
// integer), and the corrected field is 2^-k times the row sum of m against the spins as they then stand -- an
// intermediate state is a spin state too -- so every partial sum of the corrected field, in ANY order of the
// corrections, is 2^-k times an integer of magnitude at most B: exact in fp32.  The row kernel's dot for the same spins
// is the fp32 rounding of the exact row sum (int32 for int8 rows, fp32 for the integer class, fp64 in any order for the
// grid class: all exact), and that sum is representable: dot == the corrected field, bit for bit.  The
// decision is then the row kernels' own call, metropolis_accept(rule, arith, dot, s, h, 0, T, u, dE) -- Metropolis in
// either arithmetic, Glauber, heat bath; T = 0, T = inf and the 104 T cut-off with it; J_ii = 0 is the form's condition,
// so the fp32 operator's diagonal term is the row kernel's +-0 -- on the update's own u (Philox word y | w of block
// t >> 1, fetch_pair's, or replay_u), and E += dE runs in chain order.  h never enters a sum that has to be exact.  The
// accept table is not used: where the row kernel decides with it, it tabulates the same expf_det((float)(-dE / T)).
// A block decides its 64 updates against fields that hold every earlier accept; the first lane that flips is the
// chain's next flip (every lane before it stays), and the decision is a pure function of (field, spin, u, T).
// Shared-coupling batches (a.reps_per_model > 0): the product knows J and the spins only; a wave of the chain resolves
// its replica's model once and reads that model's h.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "sweep_common.h"

namespace sga {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int SEQ_TILE = 128;  // replicas x sites per workgroup (2 x 2 waves of 64 x 64, as fields_dense.hip)

struct SeqProductArgs {
    const void *J;        // [n][ldj] int8 | float
    const int8_t *spins;  // [R][sstride]
    int *base;            // [R][W]
    long long ldj;
    float scale;          // 2^k (fp32 matrix cores: the result 2^k acc is the integer D)
    int sstride, R, W;
    int t0, cnt;          // the window's first site and its sites
    int kpad, kchunk;     // columns walked (n rounded up to 32) and columns per K split (a multiple of 128)
    int ksplit, n_it, n_rt;
};

// four floats on the grid -> four int8 in one dword (element order = byte order: the K order of A and B agree)
__device__ __forceinline__ int seq_pack4(const float4 x, float scale) {
    const int a = (int)(x.x * scale), b = (int)(x.y * scale), c = (int)(x.z * scale), d = (int)(x.w * scale);
    return (a & 255) | ((b & 255) << 8) | ((c & 255) << 16) | (int)((unsigned int)d << 24);
}

// UU K steps of 32 columns from k0.  MODE 0: int8 rows on the int8 matrix cores | 1: fp32 rows on the fp32 matrix cores.
// Lane (row q, half hh) holds columns [k0 + 32 u + 16 hh, + 16) of its spin and coupling rows.
template <int MODE, int UU, typename ACC>
__device__ __forceinline__ void seq_product_steps(const int8_t *(&Sa)[2], const unsigned char *(&Jb)[2], long long k0,
                                                  int hh, ACC (&acc)[2][2]) {
    if constexpr (MODE == 0) {
        v4i fa[UU][2], fb[UU][2];
#pragma unroll
        for (int u = 0; u < UU; ++u)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const long long c = k0 + 32 * u + 16 * hh;
                fa[u][t] = *reinterpret_cast<const v4i *>(Sa[t] + c);
                fb[u][t] = *reinterpret_cast<const v4i *>(Jb[t] + c);
            }
#pragma unroll
        for (int u = 0; u < UU; ++u)
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int nn = 0; nn < 2; ++nn)
                    acc[m][nn] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[u][m], fb[u][nn], acc[m][nn], 0, 0, 0);
    } else {
        // 32 columns = four macro steps of 8: lane (row, half) holds elements [k + 4 half, + 4) of its rows and feeds
        // them to four consecutive MFMAs (fields_mfma_kernel<1>)
#pragma unroll
        for (int uu = 0; uu < UU; ++uu) {
            int sa[4][2];
            float4 xb[4][2];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const long long c = k0 + 32 * uu + 8 * u + 4 * hh;
                    sa[u][t] = *reinterpret_cast<const int *>(Sa[t] + c);
                    xb[u][t] = *reinterpret_cast<const float4 *>(Jb[t] + c * 4);
                }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float af[2][4];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    af[t][0] = (float)(int8_t)(sa[u][t]);
                    af[t][1] = (float)(int8_t)(sa[u][t] >> 8);
                    af[t][2] = (float)(int8_t)(sa[u][t] >> 16);
                    af[t][3] = (float)(sa[u][t] >> 24);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int m = 0; m < 2; ++m)
#pragma unroll
                        for (int nn = 0; nn < 2; ++nn) {
                            const float bv = e == 0 ? xb[u][nn].x : e == 1 ? xb[u][nn].y : e == 2 ? xb[u][nn].z : xb[u][nn].w;
                            acc[m][nn] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m][e], bv, acc[m][nn], 0, 0, 0);
                        }
            }
        }
    }
}

// The resident int8 copy of fp32 rows (SeqWindows::j8): one workgroup per row, four columns per thread and step.
__global__ void __launch_bounds__(256) seq_to_i8_kernel(const float *J, long long ldj, float scale, int8_t *out, long long ld8) {
    const float *row = J + (long long)blockIdx.x * ldj;
    int *dst = reinterpret_cast<int *>(out + (long long)blockIdx.x * ld8);
    for (long long c = 4 * (long long)threadIdx.x; c < ld8; c += 4 * 256)  // (ldj % 4 == 0: a load stays in the row)
        dst[c >> 2] = c < ldj ? seq_pack4(*reinterpret_cast<const float4 *>(row + c), scale) : 0;
}

hipError_t launch_seq_build_i8(const float *J, long long ldj, int n, int grid_k, int8_t *out, long long ld8, hipStream_t st) {
    if (!J || !out || n <= 0 || grid_k < 0 || grid_k > 30 || ldj % 4 != 0 || ld8 % 4 != 0 || ld8 < n || ldj < n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(seq_to_i8_kernel, dim3(n), dim3(256), 0, st, J, ldj, std::ldexp(1.0f, grid_k), out, ld8);
    return hipGetLastError();
}

// Which (replica tile, site tile, K split) a workgroup takes.  Workgroups are dealt to the 8 XCDs round robin by their
// linear id, and every XCD has its own L2 (fields_tile_of): a unit (site tile, K split) -- 128 coupling rows over one K
// range -- belongs to XCD (unit % 8), which runs the unit's replica tiles back to back, so the first of them pulls the
// rows through that L2 and the others find them there.  With the K split fastest in the unit an XCD also keeps to few K
// ranges of the spins (8 splits: one range per XCD, read from HBM once per window).
template <int MODE>
__global__ void __launch_bounds__(256) seq_product_kernel(const SeqProductArgs a) {
    using acc_t = typename std::conditional<MODE == 1, v16f, v16i>::type;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane & 31, hh = lane >> 5;
    const int L = (int)blockIdx.x, x = L & 7, slot = L >> 3;
    const int rt = slot % a.n_rt, unit = (slot / a.n_rt) * 8 + x;
    if (unit >= a.n_it * a.ksplit) return;  // (a remainder slot of the last group of 8 units)
    const int it = unit / a.ksplit, ks = unit - it * a.ksplit;
    const int kbeg = ks * a.kchunk, kend = min(a.kpad, kbeg + a.kchunk);
    const int r0 = rt * SEQ_TILE + (w >> 1) * 64;
    const int i0 = it * SEQ_TILE + (w & 1) * 64;  // (in the window)
    if (r0 >= a.R || i0 >= a.cnt || kbeg >= kend) return;  // nothing of this wave's is stored (no barrier below)
    // rows past the end are clamped for the loads (their results are not stored)
    const int8_t *Sa[2];
    const unsigned char *Jb[2];
    constexpr int JB = MODE == 0 ? 1 : 4;  // bytes per coupling
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int rr = min(r0 + 32 * t + q, a.R - 1), ii = a.t0 + min(i0 + 32 * t + q, a.cnt - 1);
        Sa[t] = a.spins + (long long)rr * a.sstride;
        Jb[t] = reinterpret_cast<const unsigned char *>(a.J) + (long long)ii * a.ldj * JB;
    }
    acc_t acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nn = 0; nn < 2; ++nn)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[m][nn][j] = 0;
    constexpr int U = MODE == 0 ? 4 : 1;  // K steps whose loads are issued together
    long long k0 = kbeg;
    for (; k0 + 32 * U <= kend; k0 += 32 * U) seq_product_steps<MODE, U>(Sa, Jb, k0, hh, acc);
    if constexpr (U > 1)
        for (; k0 < kend; k0 += 32) seq_product_steps<MODE, 1>(Sa, Jb, k0, hh, acc);
    // C/D layout of the 32x32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nn = 0; nn < 2; ++nn) {
            const int col = i0 + 32 * nn + q;
            if (col >= a.cnt) continue;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int row = r0 + 32 * m + (j & 3) + 8 * (j >> 2) + 4 * hh;
                if (row >= a.R) continue;
                int v;
                if constexpr (MODE == 1) v = (int)(acc[m][nn][j] * a.scale);  // exact: an integer below 2^24
                else v = acc[m][nn][j];
                int *dst = a.base + (long long)row * a.W + col;
                if (a.ksplit > 1) atomicAdd(dst, v);
                else *dst = v;
            }
        }
}

// ---- chain: one wave per replica, W = 64 NB pending fields ---------------------------------------------------------
constexpr int SEQ_CHAIN_K = 4;  // candidates fetched per round (rs_chain_kernel's)
constexpr int SEQ_CHAIN_U = 8;  // earlier accepts applied to a block per wait

template <typename JE, int NB>
__global__ void __launch_bounds__(64) seq_chain_kernel(const SweepArgs a, const SeqWindows sq, int k, int win) {
    constexpr int W = 64 * NB, K = SEQ_CHAIN_K, U = SEQ_CHAIN_U;
    __shared__ uint32_t alist[W + U];  // the window's accepts in chain order: site | (spin before the flip < 0) << 31
    const int r = blockIdx.x, lane = threadIdx.x, n = a.n;
    const int t0 = win * W, cnt = min(W, n - t0);
    const double T = a.sched ? a.sched[k * a.sched_ss + r * a.sched_rs] : a.rep_temp[r];
    int8_t *srow = a.spins + (long long)r * a.sstride;
    const int *base = sq.base + (long long)r * W;
    // the h of this replica's model (one matrix, many field vectors); resolved once, wave-uniform
    const float *hvec = a.h;
    if (a.reps_per_model > 0)
        hvec += (long long)__builtin_amdgcn_readfirstlane((int)((a.replica0 + (uint32_t)r) / (uint32_t)a.reps_per_model)) * n;
    const int gk = sq.grid ? sq.grid - 1 : 0;
    const float *ru = a.replay_u ? a.replay_u + (long long)r * a.replay_stride + (long long)k * n : nullptr;
    int s[NB];
    float f[NB], hh[NB], u[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int tw = 64 * b + lane, t = t0 + tw;
        const bool valid = tw < cnt;
        u[b] = 2.0f, f[b] = 0.0f, hh[b] = 0.0f, s[b] = 1;
        if (valid) {
            if (ru) {
                u[b] = ru[t];
            } else {  // update t takes word y | w of Philox block t >> 1 (fetch_pair)
                const u32x4 wd = sweep_block(a, r, k, (uint32_t)(t >> 1));
                u[b] = word_to_u((t & 1) ? wd.w : wd.y);
            }
            f[b] = ldexpf((float)base[tw], -gk);  // 2^-k D, exact
            hh[b] = hvec[t];
            s[b] = srow[t];
        }
    }
    double E = a.energy[r];
    int nA = 0;  // accepts of this window so far
    const int nblk = (cnt + 63) >> 6;
    for (int cb = 0; cb < nblk; ++cb) {
        int cs = 1;
        float cf = 0.0f, chh = 0.0f, cu = 2.0f;
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (b == cb) cs = s[b], cf = f[b], chh = hh[b], cu = u[b];
        const int ct = t0 + 64 * cb + lane;  // this lane's site
        const bool cvalid = 64 * cb + lane < cnt;
        // the lane's column in a row of J (a lane past the window's end reads the window's first column: in the row)
        const long long col = cvalid ? ct : t0;
        const JE *Jc = reinterpret_cast<const JE *>(a.J) + col;
        // The fence of the accept list: the workgroup is one wave, so no barrier is executed, but neither the compiler
        // nor the LDS queue may move the reads below ahead of lane 0's stores to alist (wave-uniform control flow).
        __syncthreads();
        for (int k0 = 0; k0 < nA; k0 += U) {
            uint32_t e[U];
            JE x[U];
#pragma unroll
            for (int j = 0; j < U; ++j) e[j] = alist[k0 + j];  // (past nA: in the array, unused)
#pragma unroll
            for (int j = 0; j < U; ++j) {
                x[j] = JE(0);
                if (k0 + j < nA) {  // wave-uniform, here and below
                    e[j] = (uint32_t)__builtin_amdgcn_readfirstlane((int)e[j]);
                    x[j] = Jc[(long long)(e[j] & 0x7fffffffu) * a.ldj];
                }
            }
#pragma unroll
            for (int j = 0; j < U; ++j)
                if (k0 + j < nA) cf -= (float)x[j] * ((e[j] >> 31) ? -2.0f : 2.0f);
        }
        double dE = 0.0;
        bool flipped = false;
        bool acc = cvalid && metropolis_accept(a.rule, a.arith, cf, cs, chh, 0.0f, T, cu, dE);
        unsigned long long m = ballot64(acc);  // flipping lanes among the undecided ones
        while (m) {
            int cl[K];
            JE x[K];
            unsigned long long rest = m;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                cl[j] = rest ? (int)__builtin_ctzll(rest) : 64;
                rest &= rest - 1;
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                x[j] = JE(0);
                if (cl[j] < 64) x[j] = Jc[(long long)(t0 + 64 * cb + cl[j]) * a.ldj];  // wave-uniform row
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (!m) break;
                const int fl = (int)__builtin_ctzll(m);
                if (fl < cl[j]) break;      // not fetched (or the candidates are used up): the next round
                if (fl > cl[j]) continue;   // candidate j flips no longer
                const int ss = read_lane(cs, fl);
                E += read_lane(dE, fl);  // metropolis_accept's dE of the flipping update, in chain order
                if (lane == 0) alist[nA] = (uint32_t)(t0 + 64 * cb + fl) | (ss < 0 ? 0x80000000u : 0u);
                ++nA;
                if (lane == fl) flipped = true;
                cf -= (float)x[j] * (2.0f * (float)ss);  // (the flipping lane's own: J_ii = 0)
                acc = cvalid && metropolis_accept(a.rule, a.arith, cf, cs, chh, 0.0f, T, cu, dE);
                m = ballot64(acc) & (~1ull << fl);
            }
        }
        if (flipped) srow[ct] = (int8_t)(-cs);  // the block's flips, one coalesced store
    }
    if (lane == 0) {
        a.energy[r] = E;
        a.n_accepted[r] += (unsigned long long)nA;
        if (t0 + cnt == n && a.energy_trace) a.energy_trace[(long long)k * a.R + r] = E;
    }
}

template <typename JE>
static hipError_t seq_chain(const SweepArgs &a, const SeqWindows &sq, int k, int win, hipStream_t st) {
    switch (sq.W) {
        case 256: hipLaunchKernelGGL((seq_chain_kernel<JE, 4>), dim3(a.R), dim3(64), 0, st, a, sq, k, win); break;
        case 512: hipLaunchKernelGGL((seq_chain_kernel<JE, 8>), dim3(a.R), dim3(64), 0, st, a, sq, k, win); break;
        case 1024: hipLaunchKernelGGL((seq_chain_kernel<JE, 16>), dim3(a.R), dim3(64), 0, st, a, sq, k, win); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The product of one window.  The K range is split so that about four workgroups per CU are in flight (W = R = 1024 has
// only 64 tiles of 128 x 128), a split never shorter than 256 columns; more than one split: base is zeroed first and
// the partial sums meet in atomics.
static hipError_t seq_product(const SweepArgs &a, const SeqWindows &sq, int cus, int win, hipStream_t st) {
    SeqProductArgs p{};
    p.J = sq.j8 ? sq.j8 : a.J;
    p.spins = a.spins;
    p.base = sq.base;
    p.ldj = sq.j8 ? sq.ld8 : a.ldj;
    p.scale = std::ldexp(1.0f, sq.grid ? sq.grid - 1 : 0);
    p.sstride = a.sstride;
    p.R = a.R;
    p.W = sq.W;
    p.t0 = win * sq.W;
    p.cnt = a.n - p.t0 < sq.W ? a.n - p.t0 : sq.W;
    p.kpad = (a.n + 31) / 32 * 32;
    p.n_it = (p.cnt + SEQ_TILE - 1) / SEQ_TILE;
    p.n_rt = (a.R + SEQ_TILE - 1) / SEQ_TILE;
    const int tiles = p.n_it * p.n_rt;
    int ks = (4 * (cus > 0 ? cus : 256) + tiles - 1) / tiles;
    if (ks > p.kpad / 256) ks = p.kpad / 256;
    if (ks < 1) ks = 1;
    p.kchunk = ((p.kpad + ks - 1) / ks + 127) / 128 * 128;
    p.ksplit = (p.kpad + p.kchunk - 1) / p.kchunk;
    if (p.ksplit > 1) {
        const hipError_t e = hipMemsetAsync(sq.base, 0, sizeof(int) * (size_t)a.R * (size_t)sq.W, st);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)(8 * ((p.n_it * p.ksplit + 7) / 8) * p.n_rt));
    switch (sq.mode) {
        case 0: hipLaunchKernelGGL(seq_product_kernel<0>, grid, dim3(256), 0, st, p); break;
        case 1: hipLaunchKernelGGL(seq_product_kernel<1>, grid, dim3(256), 0, st, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_sweep_dense_seq(const SweepArgs &a, const SeqWindows &sq, bool j_is_i8, int cus, hipStream_t st) {
    if (!a.J || !sq.base || a.rep_list || a.R <= 0 || a.n <= 0 || (sq.W != 256 && sq.W != 512 && sq.W != 1024)) return hipErrorInvalidValue;
    if (a.site_mode != SGA_SITE_SEQUENTIAL || a.accept_trace || a.dE_trace) return hipErrorInvalidValue;
    // one matrix: one model, or many field vectors over a shared one
    if (a.reps_per_model < 0 || (a.reps_per_model > 0 && a.model_stride_j != 0)) return hipErrorInvalidValue;
    if (sq.grid < 0 || sq.grid > 31 || sq.mode < 0 || sq.mode > 1 || (sq.mode == 0 && !j_is_i8 && !sq.j8) || (j_is_i8 && (sq.mode != 0 || sq.j8)) || (j_is_i8 && sq.grid > 1)) return hipErrorInvalidValue;
    // the single-site rules; Glauber and heat bath decide in fp64 only (sga_sweep refuses them fp32 arithmetic)
    if (a.rule != SGA_RULE_METROPOLIS && a.rule != SGA_RULE_GLAUBER && a.rule != SGA_RULE_HEAT_BATH) return hipErrorInvalidValue;
    if (a.rule != SGA_RULE_METROPOLIS && a.arith != SGA_ARITH_F64) return hipErrorInvalidValue;
    // the product walks whole K steps of 32 columns with 16-byte loads: inside the rows' strides (zero padded)
    const long long kpad = ((long long)a.n + 31) / 32 * 32;
    if (a.sstride % 16 != 0 || a.sstride < kpad || a.ldj < kpad || a.ldj % (j_is_i8 ? 16 : 4) != 0) return hipErrorInvalidValue;
    if ((long long)a.R * a.n >= (1ll << 31)) return hipErrorInvalidValue;
    if (sq.j8 && (sq.mode != 0 || sq.ld8 < kpad || sq.ld8 % 16 != 0)) return hipErrorInvalidValue;
    const int nwin = (a.n + sq.W - 1) / sq.W;
    hipError_t e = hipSuccess;
    for (int k = 0; k < a.n_sweeps && e == hipSuccess; ++k) {
        for (int w = 0; w < nwin && e == hipSuccess; ++w) {
            e = seq_product(a, sq, cus, w, st);
            if (e != hipSuccess) break;
            e = j_is_i8 ? seq_chain<int8_t>(a, sq, k, w, st) : seq_chain<float>(a, sq, k, w, st);
        }
        // sweep boundary: best tracking (annealing/gpu_annealer.py:151-153), the energy is in a.energy
        if (e == hipSuccess && !a.no_best)
            e = launch_update_best(a.energy, a.spins, a.best_energy, a.best_spins, a.sstride, a.R, st);
    }
    if (e == hipSuccess) {
        char gs[64] = "";
        if (sq.grid) std::snprintf(gs, sizeof(gs), ", grid=2^-%d", sq.grid - 1);
        if (a.rule != SGA_RULE_METROPOLIS)
            std::snprintf(gs + std::strlen(gs), sizeof(gs) - std::strlen(gs), ", rule=%s", a.rule == SGA_RULE_GLAUBER ? "glauber" : "heat-bath");
        note_sweep_kernel("sweep_dense_seq<%s, W=%d%s> (sequential windows: product on %s matrix cores, chain)",
                          j_is_i8 ? "int8_t" : "float", sq.W, gs, sq.mode == 1 ? "f32" : "i8");
    }
    return e;
}

}  // namespace sga
