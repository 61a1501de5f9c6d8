// resample.hip -- the resampling step of population annealing (Hukushima and Iba 2003; Machta 2010; Wang, Machta and
// Katzgraber 2015): sga_resample.  The rule stands in sga_replicas.h (ResampleArgs): weights as 40-bit fixed point, one
// 64-bit draw per population (sweep_common.h, resample_draw), systematic resampling in 128-bit integer compares,
// survivors keep their slots.  Integer sums are exact in any order, so the plan is a function of the energies, dbeta,
// the seed and the round alone, whatever the launch shape.
//
// Plan kernel: one workgroup of 256 threads per population, thread t owning the members [t chunk, (t + 1) chunk).  Three
// walks over the members with a workgroup scan between them:
//   A  x_max (a workgroup max), then W_r into C[] and the thread's sum;            scan: the sums of W  -> S, the offset o
//   B  C_r in place, F_r = #{k : k S + o < N C_r} (a search over k, 24 steps at   scan: the threads' slots with no child
//      most), so n_r = F_r - F_{r-1}, and the thread's count of n_r == 0;
//   C  SP_r = the surplus copies of members 0 ... r = F_r - (r + 1) + Z_r, and the rank of every slot without a child;
//   D  (members strided) the j-th slot without a child takes the j-th entry of the surplus list: the smallest r with
//      SP_r > j, a search over SP[]; with it the flag of the best (sga_replicas.h, take_best).
// Copy kernel: a workgroup per overwritten slot and 16 KiB of its row, 16 bytes a lane and access; the first of a slot
// also moves the energy and the best energy.  It reads parent[] and take_best[] only, which it never writes.
#include "sweep_common.h"

namespace sga {

namespace {

using u64 = unsigned long long;

// exclusive prefix of v over the workgroup's 256 threads and the total (sh: 512 entries; Hillis-Steele, two buffers)
template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *sh, T &total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    int in = 0;
    for (int d = 1; d < RESAMPLE_THREADS; d <<= 1) {
        T x = sh[in * RESAMPLE_THREADS + t];
        if (t >= d) x += sh[in * RESAMPLE_THREADS + t - d];
        in ^= 1;
        sh[in * RESAMPLE_THREADS + t] = x;
        __syncthreads();
    }
    const T incl = sh[in * RESAMPLE_THREADS + t];
    total = sh[in * RESAMPLE_THREADS + RESAMPLE_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// #{k in [0, N) : k S + o < N C}: the children whose position lies below N C (monotone in k: a search)
__device__ __forceinline__ int children_below(u64 C, u64 S, u64 o, int N) {
    const u64 rhs_lo = (u64)N * C, rhs_hi = __umul64hi((u64)N, C);
    int lo = 0, hi = N;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const u64 l = (u64)mid * S + o;
        const u64 h = __umul64hi((u64)mid, S) + (l < o ? 1ull : 0ull);
        if (h < rhs_hi || (h == rhs_hi && l < rhs_lo))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

}  // namespace

__global__ void __launch_bounds__(RESAMPLE_THREADS) resample_plan_kernel(const ResampleArgs a) {
    __shared__ u64 sh[2 * RESAMPLE_THREADS];
    const int tid = threadIdx.x, p = blockIdx.x, N = a.N;
    if (p >= a.n_pop) return;
    const long long base = (long long)p * N;
    const double *E = a.energy + base;
    u64 *C = a.C + base;
    int *F = a.F + base, *SP = a.SP + base;
    int32_t *par = a.parent + base;
    const int chunk = (N + RESAMPLE_THREADS - 1) / RESAMPLE_THREADS;
    const int r0 = min(N, tid * chunk), r1 = min(N, r0 + chunk);
    const double nb = -a.dbeta[p];

    // A. the largest exponent: every thread starts from member 0's, so an idle thread adds nothing
    double xm = nb * E[0];
    for (int r = r0; r < r1; ++r) {
        const double x = nb * E[r];
        xm = x > xm ? x : xm;
    }
    {
        double *shd = reinterpret_cast<double *>(sh);
        shd[tid] = xm;
        __syncthreads();
        for (int d = RESAMPLE_THREADS / 2; d > 0; d >>= 1) {
            if (tid < d) {
                const double y = shd[tid + d];
                if (y > shd[tid]) shd[tid] = y;
            }
            __syncthreads();
        }
        xm = shd[0];
        __syncthreads();
    }
    u64 mine = 0;
    for (int r = r0; r < r1; ++r) {
        const double w = exp_det(nb * E[r] - xm) * 0x1.0p40;  // in [0, 2^40]: the product exact, the cast truncating
        const u64 W = w >= 0.0 ? (u64)w : 0ull;               // (a NaN energy weighs nothing)
        C[r] = W;
        mine += W;
    }
    u64 S = 0;
    u64 c = block_exclusive_scan<u64>(mine, sh, S);
    const u64 U = resample_draw(a.round, a.gpop0 + (uint32_t)p, a.seed_lo, a.seed_hi);
    const u64 o = __umul64hi(U, S);
    if (tid == 0) {
        a.shift[p] = xm;
        a.sum[p] = S;
    }

    // B. inclusive sums in place, children up to and including r, this thread's slots without a child
    const int f_first = children_below(c, S, o, N);
    int f_prev = f_first, zeros = 0;
    for (int r = r0; r < r1; ++r) {
        c += C[r];
        C[r] = c;
        const int f = children_below(c, S, o, N);
        F[r] = f;
        zeros += f == f_prev;
        f_prev = f;
    }
    int *shi = reinterpret_cast<int *>(sh);
    int z_total = 0;
    int z = block_exclusive_scan<int>(zeros, shi, z_total);

    // C. surplus copies up to and including r; a slot without a child leaves its rank among those in par[], any other -1
    f_prev = f_first;
    for (int r = r0; r < r1; ++r) {
        const int f = F[r];
        const bool none = f == f_prev;
        par[r] = none ? z : -1;
        z += none;
        SP[r] = f - (r + 1) + z;
        f_prev = f;
    }
    __syncthreads();  // (SP[] and par[] are read across threads below)

    // D. parents: the j-th slot without a child takes entry j of the surplus list
    for (int d = tid; d < N; d += RESAMPLE_THREADS) {
        const int j = par[d];
        int src = d;
        if (j >= 0) {
            int lo = 0, hi = N;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (SP[mid] > j)
                    hi = mid;
                else
                    lo = mid + 1;
            }
            if (lo < N) src = lo;  // (always, for finite energies: the surplus list has as many entries as there are empty slots)
        }
        par[d] = (int32_t)(base + src);
        a.take_best[base + d] = (src != d && E[src] < a.best_energy[base + d]) ? 1 : 0;
    }
}

__global__ void __launch_bounds__(RESAMPLE_THREADS) resample_copy_kernel(const int32_t *parent, const int *take_best, int8_t *spins,
                                                                         double *energy, int8_t *best_spins, double *best_energy,
                                                                         int sstride, int R, int pieces) {
    const int d = blockIdx.x / pieces, piece = blockIdx.x % pieces;
    if (d >= R) return;
    const int src = parent[d];
    if (src == d || src < 0 || src >= R) return;  // uniform per workgroup: a survivor, or an untouched slot
    const bool best = take_best[d] != 0;
    const int i0 = piece * (RESAMPLE_COPY_BYTES / 16), i1 = min(sstride / 16, i0 + RESAMPLE_COPY_BYTES / 16);
    const int4 *from = reinterpret_cast<const int4 *>(spins + (long long)src * sstride);
    int4 *to = reinterpret_cast<int4 *>(spins + (long long)d * sstride);
    int4 *to_best = reinterpret_cast<int4 *>(best_spins + (long long)d * sstride);
    for (int i = i0 + threadIdx.x; i < i1; i += RESAMPLE_THREADS) {
        const int4 v = from[i];
        to[i] = v;
        if (best) to_best[i] = v;
    }
    if (piece == 0 && threadIdx.x == 0) {
        const double e = energy[src];  // (a survivor's: nothing writes it)
        energy[d] = e;
        if (best) best_energy[d] = e;
    }
}

hipError_t launch_resample_plan(const ResampleArgs &a, hipStream_t st) {
    if (a.n_pop <= 0 || a.N <= 0 || a.N > RESAMPLE_MAX_MEMBERS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resample_plan_kernel, dim3(a.n_pop), dim3(RESAMPLE_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_resample_copy(const int32_t *parent, const int *take_best, int8_t *spins, double *energy, int8_t *best_spins,
                                double *best_energy, int sstride, int R, hipStream_t st) {
    if (R <= 0 || sstride <= 0 || sstride % 16 != 0) return hipErrorInvalidValue;
    const long long pieces = ((long long)sstride + RESAMPLE_COPY_BYTES - 1) / RESAMPLE_COPY_BYTES;
    if (pieces * R > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resample_copy_kernel, dim3((unsigned)(pieces * R)), dim3(RESAMPLE_THREADS), 0, st, parent, take_best, spins,
                       energy, best_spins, best_energy, sstride, R, (int)pieces);
    return hipGetLastError();
}

}  // namespace sga
