// pair_overlaps.hip -- spin and link overlaps between pairs of replicas, measured where the spins are:
// sga_get_pair_overlaps / sga_accumulate_ladder_overlaps / sga_get_link_count.
//
// For a pair (a, b) with x_i = [s_a[i] != s_b[i]]: d = sum_i x_i (n q_ab = n - 2 d), and over the links of the stored
// rows -- the entries cluster_moves_kernel follows: value not +-0, j != i, 0 <= j < n, both triangles -- b = the number
// with x_i != x_j (L q_l = L - 2 b).  Everything is an integer count: the result does not depend on any order.
//
// Mapping: one workgroup of 256 threads per pair.  1. the diff words, 16 sites a load, popcounted into d and, with links
// asked for, kept as a bitmap of ceil(n / 32) words in LDS; 2. groups of 2^g lanes take a row each and walk it 2^g
// entries a step (8-byte loads, coalesced within the group), g chosen per launch from the layout's mean row
// (pair_overlap_group_log2); every lane counts into a 64-bit register, the workgroup adds them up in 64 bits; 3. one
// thread stores d and b, or bumps the pair's cell of the caller's histograms (one workgroup owns one cell per launch:
// a plain 64-bit load / add / store).  No loop depends on the data: n rows, the layout's entries.
#include "sweep_common.h"

namespace sga {

namespace {

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the sums of v over the workgroup's 256 threads, in every thread (red: 4 words of LDS; two barriers)
__device__ __forceinline__ int block_sum(int v, int *red) {
    const int w = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    const int t = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return t;
}
__device__ __forceinline__ unsigned long long block_sum64(unsigned long long v, unsigned long long *red) {
    const unsigned long long w = wave_sum64(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    const unsigned long long t = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return t;
}

// Over the rows row0, row0 + row_step, ...: the links -- all of them, or (DIFF) those whose ends differ in x
template <bool DIFF>
__device__ __forceinline__ unsigned long long walk_links(const long long *rowptr64, const int2 *cv, int n, int glog,
                                                         long long row0, long long row_step, const unsigned int *x) {
    const int G = 1 << glog, gl = threadIdx.x & (G - 1);
    unsigned long long mine = 0;
    for (long long r = row0; r < n; r += row_step) {
        const int i = (int)r;
        const long long beg = rowptr64[i], end = rowptr64[i + 1];
        const unsigned int xi = DIFF ? x[i >> 5] >> (i & 31) : 0u;
        for (long long e = beg + gl; e < end; e += G) {
            const int2 ent = cv[e];
            const int j = ent.x;
            if ((ent.y & 0x7fffffff) == 0 || j == i || (unsigned)j >= (unsigned)n) continue;  // cluster_moves_kernel's link
            mine += DIFF ? (unsigned long long)((xi ^ (x[j >> 5] >> (j & 31))) & 1u) : 1ull;
        }
    }
    return mine;
}

}  // namespace

__global__ void __launch_bounds__(PAIR_OVERLAP_THREADS) pair_overlaps_kernel(const PairOverlapArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = a.n, tid = threadIdx.x, p = blockIdx.x;
    const int words = (n + 31) / 32;
    int *red = reinterpret_cast<int *>(smem);                                          // [0..3]
    unsigned long long *red64 = reinterpret_cast<unsigned long long *>(smem + 16);     // [0..3]
    unsigned int *diff = reinterpret_cast<unsigned int *>(smem + PAIR_OVERLAP_LDS_FIXED);  // links only

    int ra, rb;
    if (a.pairs) {
        ra = a.pairs[2 * p];
        rb = a.pairs[2 * p + 1];
    } else {  // ladders 2c and 2c + 1, one slot: the replicas that hold it now
        const int c = p / a.n_slots, s = a.slot_lo + p % a.n_slots;
        ra = a.slot_to_rep[(long long)(2 * c) * a.L + s] - a.replica0;
        rb = a.slot_to_rep[(long long)(2 * c + 1) * a.L + s] - a.replica0;
    }
    if (ra < 0 || ra >= a.R || rb < 0 || rb >= a.R) return;  // (never, after the host's checks: no access at all then)
    const int8_t *sa = a.spins + (long long)ra * a.sstride;
    const int8_t *sb = a.spins + (long long)rb * a.sstride;

    // 1. diff, 16 sites a load; a word's second half is read only where it holds a site (rows end at a multiple of 16)
    int mine = 0;
    for (int w = tid; w < words; w += PAIR_OVERLAP_THREADS) {
        const int i0 = 32 * w;
        unsigned int b = diff_bits16(*reinterpret_cast<const int4 *>(sa + i0), *reinterpret_cast<const int4 *>(sb + i0));
        if (i0 + 16 < n)
            b |= diff_bits16(*reinterpret_cast<const int4 *>(sa + i0 + 16), *reinterpret_cast<const int4 *>(sb + i0 + 16)) << 16;
        if (n - i0 < 32) b &= (1u << (n - i0)) - 1u;  // the pad past n is no site
        if (a.links) diff[w] = b;
        mine += __popc(b);
    }
    const int d = block_sum(mine, red);  // (its barriers order the bitmap's stores before the walk)

    // 2. the broken links; identical configurations break none (d is the same in every thread)
    unsigned long long broken = 0;
    if (a.links && d > 0) {
        const int glog = a.group_log2;
        broken = block_sum64(walk_links<true>(a.rowptr64, a.cv, n, glog, tid >> glog, PAIR_OVERLAP_THREADS >> glog, diff), red64);
    }

    // 3. one thread stores
    if (tid != 0) return;
    if (a.pairs) {
        if (a.dist) a.dist[p] = d;
        if (a.broken) a.broken[p] = (long long)broken;
        return;
    }
    const unsigned int bq = min((unsigned int)d >> a.q_shift, (unsigned int)(a.bins_q - 1));
    a.hist_q[(size_t)p * (size_t)a.bins_q + bq] += 1ull;
    if (a.hist_l) {
        const unsigned long long bl = min(broken >> a.l_shift, (unsigned long long)(a.bins_l - 1));
        a.hist_l[(size_t)p * (size_t)a.bins_l + bl] += 1ull;
    }
}

// every workgroup takes rows in a grid stride and adds its count to *out
__global__ void __launch_bounds__(PAIR_OVERLAP_THREADS) link_count_kernel(const long long *rowptr64, const int2 *cv, int n, int glog,
                                                                          unsigned long long *out) {
    __shared__ unsigned long long red64[4];
    const long long groups = PAIR_OVERLAP_THREADS >> glog;
    const unsigned long long c = block_sum64(
        walk_links<false>(rowptr64, cv, n, glog, (long long)blockIdx.x * groups + (threadIdx.x >> glog), (long long)gridDim.x * groups, nullptr),
        red64);
    if (threadIdx.x == 0 && c) atomicAdd(out, c);
}

hipError_t launch_pair_overlaps(const PairOverlapArgs &a, hipStream_t st) {
    if (a.count <= 0) return hipSuccess;
    const size_t lds = pair_overlap_lds_bytes(a.n, a.links != 0);
    if (a.n <= 0 || lds > CLUSTER_LDS_BUDGET || a.sstride % 16 != 0 || a.sstride < a.n || a.group_log2 < 0 || a.group_log2 > 6)
        return hipErrorInvalidValue;
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(pair_overlaps_kernel), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pair_overlaps_kernel, dim3(a.count), dim3(PAIR_OVERLAP_THREADS), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_link_count(const long long *rowptr64, const int2 *cv, int n, int group_log2, unsigned long long *out,
                             hipStream_t st) {
    if (n <= 0 || group_log2 < 0 || group_log2 > 6) return hipErrorInvalidValue;
    const long long groups = PAIR_OVERLAP_THREADS >> group_log2;
    const int blocks = (int)std::min<long long>((n + groups - 1) / groups, 4096);
    hipLaunchKernelGGL(link_count_kernel, dim3(blocks), dim3(PAIR_OVERLAP_THREADS), 0, st, rowptr64, cv, n, group_log2, out);
    return hipGetLastError();
}

}  // namespace sga
