// observables.hip -- replica observables on the device (DESIGN.md "Replica observables"; sga_get_magnetizations,
// sga_get_overlaps, sga_get_overlaps_with).
//
// One product serves them all: Q = A B^T, A the replicas' int8 spins [rows_a][lda] (current or best), B a set of int8
// configurations [rows_b][ldb] -- the same spins (overlap matrix), the best configurations (distances between
// solutions), rows the caller hands over (a planted state, another rank's spins).  Sites are the columns 0 ... n - 1.
//
// Operands.  v_mfma_i32_32x32x32_i8 takes, from lane (q = lane & 31, hh = lane >> 5), 16 consecutive K elements
// [k0 + 16 hh, + 16) of row q of A and of row q of B (the layout of seq_product_kernel, sweep_dense_seq.hip): both
// operands are read straight from their row-major rows, 16 contiguous bytes per lane and K step, no LDS and no
// transpose.  Result register j of that lane is Q[row (j & 3) + 8 (j >> 2) + 4 hh][column q].
//
// Exactness.  Products of int8 values and their int32 sums are integer arithmetic: |any partial sum| <= 127 * 127 n,
// and for spins (|s| <= 1) against int8 rows <= 127 n < 2^31 for every n a spin row can have.  A K range's partial sum
// is one such sum, and int32 atomicAdd is associative and commutative: Q is the exact product whatever the split and
// the order in which the workgroups arrive.  Bit for bit numpy's int64 product.
//
// Sites k >= n are masked in the kernel, not trusted to be zero: a K range ends at n, its whole K steps lie below n,
// and the last, partial step loads byte by byte under k < n.  Rows past rows_a / rows_b are clamped for the loads and
// predicated on the store.
//
// A is B (sga_get_overlaps with which_a == which_b): only the tiles with a <= b are computed.  A tile off the diagonal
// writes its mirror image too, each 32 x 32 result turned through LDS first so that the lanes of a store run along a
// row of the result (as the registers lie they would run down a column: 32 cache lines per instruction instead of 2;
// measured at n = 10^4, R = 1024: 0.142 -> 0.087 ms per call).
//
// No Philox call: nothing here draws a random number.
#include "sga_replicas.h"

namespace sga {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// 16 K elements [c, c + 16) of a row, zero where k >= n: byte loads, any alignment
__device__ __forceinline__ v4i obs_load_guarded(const int8_t *row, long long c, int n) {
    v4i v;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        unsigned int w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long long k = c + 4 * d + b;
            const unsigned int x = k < n ? (unsigned int)(unsigned char)row[k] : 0u;
            w |= x << (8 * b);
        }
        v[d] = (int)w;
    }
    return v;
}

// UU K steps of 32 columns from k0 (all below n).  VEC: 16-byte loads (rows 16-byte aligned, k0 a multiple of 32).
template <bool VEC, int UU>
__device__ __forceinline__ void obs_steps(const int8_t *(&Ar)[2], const int8_t *(&Br)[2], long long k0, int hh, int n,
                                          v16i (&acc)[2][2]) {
    v4i fa[UU][2], fb[UU][2];
#pragma unroll
    for (int u = 0; u < UU; ++u)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const long long c = k0 + 32 * u + 16 * hh;
            if constexpr (VEC) {
                fa[u][t] = *reinterpret_cast<const v4i *>(Ar[t] + c);
                fb[u][t] = *reinterpret_cast<const v4i *>(Br[t] + c);
            } else {
                fa[u][t] = obs_load_guarded(Ar[t], c, n);
                fb[u][t] = obs_load_guarded(Br[t], c, n);
            }
        }
#pragma unroll
    for (int u = 0; u < UU; ++u)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int nn = 0; nn < 2; ++nn)
                acc[m][nn] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[u][m], fb[u][nn], acc[m][nn], 0, 0, 0);
}

// grid (tiles_n, tiles_m, ksplit), 256 threads: wave w takes rows [64 (w >> 1), + 64) of the A tile against rows
// [64 (w & 1), + 64) of the B tile, as 2 x 2 products of 32 x 32.
template <bool VEC>
__global__ void __launch_bounds__(256) observables_product_kernel(const ObservablesArgs a) {
    const int tn = (int)blockIdx.x, tm = (int)blockIdx.y, ks = (int)blockIdx.z;
    if (a.symmetric && tm > tn) return;  // the mirror image of tile (tn, tm), which writes both halves
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane & 31, hh = lane >> 5;
    const int r0 = tm * OBS_TILE + (w >> 1) * 64;
    const int c0 = tn * OBS_TILE + (w & 1) * 64;
    const int kbeg = ks * a.plan.kchunk;
    const int kend = min(a.n, kbeg + a.plan.kchunk);
    if (r0 >= a.rows_a || c0 >= a.rows_b || kbeg >= kend) return;  // nothing of this wave's is stored (no barrier below)
    const int8_t *Ar[2], *Br[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        Ar[t] = a.A + (long long)min(r0 + 32 * t + q, a.rows_a - 1) * a.lda;
        Br[t] = a.B + (long long)min(c0 + 32 * t + q, a.rows_b - 1) * a.ldb;
    }
    v16i acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nn = 0; nn < 2; ++nn)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[m][nn][j] = 0;
    long long k0 = kbeg;
    if constexpr (VEC)  // (byte loads: one K step at a time, 128 byte loads in flight are enough)
        for (; k0 + 128 <= kend; k0 += 128) obs_steps<VEC, 4>(Ar, Br, k0, hh, a.n, acc);
    for (; k0 + 32 <= kend; k0 += 32) obs_steps<VEC, 1>(Ar, Br, k0, hh, a.n, acc);
    if (k0 < kend) obs_steps<false, 1>(Ar, Br, k0, hh, a.n, acc);  // the step that holds n: masked byte by byte
    const bool mirror = a.symmetric && tm != tn;
    const bool joined = a.plan.ksplit > 1;
    __shared__ int turned[4][32][33];  // per wave: a 32 x 32 result turned for the mirror's stores (33: no bank conflicts)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nn = 0; nn < 2; ++nn) {
            const int col = c0 + 32 * nn + q;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int row = r0 + 32 * m + (j & 3) + 8 * (j >> 2) + 4 * hh;
                if (col >= a.rows_b || row >= a.rows_a) continue;
                int *dst = a.out + (long long)row * a.ldq + col;
                if (joined) atomicAdd(dst, acc[m][nn][j]);
                else *dst = acc[m][nn][j];
            }
            if (!mirror) continue;  // (uniform over the workgroup)
            // The other half, out[col][row]: as the registers lie, a store instruction would touch 32 rows of the result.
            // Through LDS the lanes run along the row index instead: two rows of 32 consecutive words per instruction.
            // LDS operations of one wave complete in order; the fences keep the compiler from moving them.
#pragma unroll
            for (int j = 0; j < 16; ++j) turned[w][q][(j & 3) + 8 * (j >> 2) + 4 * hh] = acc[m][nn][j];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int mc = c0 + 32 * nn + 2 * i + hh, mr = r0 + 32 * m + q;
                const int v = turned[w][2 * i + hh][q];
                if (mc >= a.rows_b || mr >= a.rows_a) continue;
                int *dst = a.out + (long long)mc * a.ldq + mr;
                if (joined) atomicAdd(dst, v);
                else *dst = v;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
        }
}

static bool obs_aligned(const void *p, long long ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 15) == 0; }

hipError_t launch_observables_product(const ObservablesArgs &a, hipStream_t st) {
    const ObservablesPlan &p = a.plan;
    if (!a.A || !a.B || !a.out || a.n <= 0 || a.rows_a <= 0 || a.rows_b <= 0 || a.lda < a.n || a.ldb < a.n || a.ldq < a.rows_b)
        return hipErrorInvalidValue;
    if (p.tiles_m != (a.rows_a + OBS_TILE - 1) / OBS_TILE || p.tiles_n != (a.rows_b + OBS_TILE - 1) / OBS_TILE || p.ksplit < 1 ||
        p.kchunk < 1 || p.kchunk % OBS_K_GRAIN != 0 || (long long)p.ksplit * p.kchunk < a.n || p.tiles_m > 65535 || p.ksplit > 65535)
        return hipErrorInvalidValue;
    if (a.symmetric && (a.A != a.B || a.lda != a.ldb || a.rows_a != a.rows_b)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)p.tiles_n, (unsigned)p.tiles_m, (unsigned)p.ksplit);
    if (obs_aligned(a.A, a.lda) && obs_aligned(a.B, a.ldb))
        hipLaunchKernelGGL(observables_product_kernel<true>, grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(observables_product_kernel<false>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---- magnetisations: a plain reduction, one workgroup per row (B = a row of ones would cost a product launch and a
// zeroing pass for a sum a wave forms in registers)
__device__ __forceinline__ int obs_byte_sum(int x) { return (int)(int8_t)x + (int)(int8_t)(x >> 8) + (int)(int8_t)(x >> 16) + (x >> 24); }

__global__ void __launch_bounds__(256) observables_row_sums_kernel(const int8_t *S, long long ld, int n, int vec, int *out) {
    __shared__ int part[4];
    const int8_t *row = S + (long long)blockIdx.x * ld;
    const int tid = threadIdx.x;
    int sum = 0;
    for (long long c = 16ll * tid; c < n; c += 16 * 256) {
        v4i v;
        if (vec && c + 16 <= n) v = *reinterpret_cast<const v4i *>(row + c);
        else v = obs_load_guarded(row, c, n);
        sum += obs_byte_sum(v[0]) + obs_byte_sum(v[1]) + obs_byte_sum(v[2]) + obs_byte_sum(v[3]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((tid & 63) == 0) part[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) out[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

hipError_t launch_observables_row_sums(const int8_t *S, long long ld, int n, int R, int *out, hipStream_t st) {
    if (!S || !out || n <= 0 || R <= 0 || ld < n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(observables_row_sums_kernel, dim3((unsigned)R), dim3(256), 0, st, S, ld, n, obs_aligned(S, ld) ? 1 : 0, out);
    return hipGetLastError();
}

}  // namespace sga
