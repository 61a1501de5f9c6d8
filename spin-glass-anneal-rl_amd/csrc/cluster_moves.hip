// cluster_moves.hip -- isoenergetic cluster moves between two replicas of one sparse Hamiltonian (Houdayer 2001;
// Zhu, Ochoa and Katzgraber 2015): sga_cluster_move_pairs / sga_cluster_move_ladders.
//
// For a pair (a, b): the sites where the two replicas differ, one of them drawn uniformly, the connected component of
// differing sites around it (connected through stored non-zero couplings), flipped in both replicas.  On the component
// the move swaps the two configurations, and every coupling that leaves the component ends on a site where the
// replicas agree, so E_a + E_b is conserved for any J and h: no accept test.  The move is a function of the two
// configurations, the graph and one Philox word (sweep_common.h, cluster_seed_word).
//
// Mapping: one workgroup of 256 threads per pair.  Four bitmaps of ceil(n / 32) words in LDS -- diff, cluster, the
// current and the next frontier -- and CLUSTER_LDS_FIXED bytes beside them; the spins stay in HBM.  The search is
// level synchronous: a group of 16 lanes takes one frontier site at a time and walks its row 16 entries a step (a hub
// of several hundred entries is 16 lanes' work, a lattice row of six one step), bits join `cluster` and the next
// frontier through LDS atomics, and a flag in LDS tells every thread behind a barrier whether another level follows.
// No input makes the loop run on: it is bounded by n levels, and every level but the last adds a site.
#include "sweep_common.h"

namespace sga {

namespace {

constexpr int CLUSTER_GROUP = 16;  // lanes that share one row

// the sum of v over the workgroup's 256 threads, in every thread (red: 4 ints of LDS; two barriers)
__device__ __forceinline__ int block_sum(int v, int *red) {
    const int w = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    const int t = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return t;
}

}  // namespace

__global__ void __launch_bounds__(CLUSTER_THREADS) cluster_moves_kernel(const ClusterArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = a.n, tid = threadIdx.x, p = blockIdx.x;
    const int words = (n + 31) / 32;
    unsigned int *diff = reinterpret_cast<unsigned int *>(smem);
    unsigned int *cluster = diff + words;
    unsigned int *cur = cluster + words;
    unsigned int *nxt = cur + words;
    int *fixed = reinterpret_cast<int *>(nxt + words);  // [0..3] wave sums, [4..7] wave prefixes, [9] the level's flag

    int ra, rb;
    if (a.pairs) {
        ra = a.pairs[2 * p];
        rb = a.pairs[2 * p + 1];
    } else {  // ladders 2c and 2c + 1, one slot: the replicas that hold it now
        const int c = p / a.n_slots, s = a.slot_lo + p % a.n_slots;
        ra = a.slot_to_rep[(long long)(2 * c) * a.L + s] - (int)a.replica0;
        rb = a.slot_to_rep[(long long)(2 * c + 1) * a.L + s] - (int)a.replica0;
    }
    if (ra < 0 || ra >= a.R || rb < 0 || rb >= a.R || ra == rb) {  // (never, after the host's checks: no access at all then)
        if (tid == 0 && a.sizes) a.sizes[p] = 0;
        return;
    }
    int8_t *sa = a.spins + (long long)ra * a.sstride;
    int8_t *sb = a.spins + (long long)rb * a.sstride;

    // 1. diff, 16 sites a load; a word's second half is read only where it holds a site (rows end at a multiple of 16)
    int mine = 0;
    for (int w = tid; w < words; w += CLUSTER_THREADS) {
        const int i0 = 32 * w;
        unsigned int b = diff_bits16(*reinterpret_cast<const int4 *>(sa + i0), *reinterpret_cast<const int4 *>(sb + i0));
        if (i0 + 16 < n)
            b |= diff_bits16(*reinterpret_cast<const int4 *>(sa + i0 + 16), *reinterpret_cast<const int4 *>(sb + i0 + 16)) << 16;
        if (n - i0 < 32) b &= (1u << (n - i0)) - 1u;  // the pad past n is no site
        diff[w] = b;
        cluster[w] = 0u;
        cur[w] = 0u;
        nxt[w] = 0u;
        mine += __popc(b);
    }
    if (tid == 0) fixed[9] = 0;
    const int count = block_sum(mine, fixed);  // (its barriers order the bitmaps' stores before what follows)
    if (count == 0) {
        if (tid == 0 && a.sizes) a.sizes[p] = 0;
        return;
    }

    // 2. the seed: the k-th set bit of diff in index order.  Thread t counts the words [t chunk, (t + 1) chunk).
    const uint32_t k = __umulhi(cluster_seed_word(a.round, a.replica0 + (uint32_t)ra, a.replica0 + (uint32_t)rb, a.seed_lo, a.seed_hi),
                                (uint32_t)count);
    {
        const int chunk = (words + CLUSTER_THREADS - 1) / CLUSTER_THREADS;
        const int w0 = min(words, tid * chunk), w1 = min(words, w0 + chunk);
        int c = 0;
        for (int w = w0; w < w1; ++w) c += __popc(diff[w]);
        int incl = c;  // inclusive prefix over the wave
        const int lane = tid & 63;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) fixed[4 + (tid >> 6)] = incl;
        __syncthreads();
        int before = incl - c;
        for (int v = 0; v < (tid >> 6); ++v) before += fixed[4 + v];
        if ((uint32_t)before <= k && k < (uint32_t)(before + c)) {  // exactly one thread
            int left = (int)k - before;
            for (int w = w0; w < w1; ++w) {
                unsigned int b = diff[w];
                const int pc = __popc(b);
                if (left >= pc) {
                    left -= pc;
                    continue;
                }
                for (; left > 0; --left) b &= b - 1u;  // (its lowest set bit is the drawn site now)
                cluster[w] = b & (0u - b);
                cur[w] = b & (0u - b);
                break;
            }
        }
        __syncthreads();
    }

    // 3. level-synchronous breadth-first search over the differing sites
    const int group = tid / CLUSTER_GROUP, gl = tid % CLUSTER_GROUP;
    constexpr int GROUPS = CLUSTER_THREADS / CLUSTER_GROUP;
    for (int level = 0; level < n; ++level) {
        for (int w = group; w < words; w += GROUPS) {
            unsigned int f = cur[w];  // (the same word in all 16 lanes)
            while (f) {
                const int i = 32 * w + (__ffs((int)f) - 1);
                f &= f - 1u;
                const long long beg = a.rowptr64[i], end = a.rowptr64[i + 1];
                for (long long e = beg + gl; e < end; e += CLUSTER_GROUP) {
                    const int2 ent = a.cv[e];
                    const int j = ent.x;
                    if ((ent.y & 0x7fffffff) == 0 || j == i || (unsigned)j >= (unsigned)n) continue;
                    const unsigned int bit = 1u << (j & 31);
                    if (!(diff[j >> 5] & bit) || (cluster[j >> 5] & bit)) continue;
                    if (!(atomicOr(&cluster[j >> 5], bit) & bit)) {
                        atomicOr(&nxt[j >> 5], bit);
                        fixed[9] = 1;
                    }
                }
            }
        }
        __syncthreads();
        const int more = fixed[9];
        __syncthreads();
        if (!more) break;
        unsigned int *t = cur;
        cur = nxt;
        nxt = t;
        for (int w = tid; w < words; w += CLUSTER_THREADS) nxt[w] = 0u;
        if (tid == 0) fixed[9] = 0;
        __syncthreads();
    }

    // 4. flip the cluster in both replicas (byte stores, a site a lane), report its size
    int size = 0;
    for (int w = tid; w < words; w += CLUSTER_THREADS) size += __popc(cluster[w]);
    for (int i = tid; i < n; i += CLUSTER_THREADS)
        if ((cluster[i >> 5] >> (i & 31)) & 1u) {
            sa[i] = (int8_t)(-sa[i]);
            sb[i] = (int8_t)(-sb[i]);
        }
    size = block_sum(size, fixed);
    if (tid == 0) {
        if (a.sizes) a.sizes[p] = size;
        a.n_accepted[ra] += (unsigned long long)size;
        a.n_accepted[rb] += (unsigned long long)size;
        a.touched[ra] = 1;
        a.touched[rb] = 1;
    }
}

__global__ void __launch_bounds__(256) cluster_finish_kernel(const int *touched, const double *saved_energy, double *energy,
                                                             const int8_t *spins, double *best_energy, int8_t *best_spins,
                                                             int sstride, int R) {
    const int r = blockIdx.x;
    if (r >= R) return;
    if (!touched[r]) {  // uniform per workgroup
        if (threadIdx.x == 0) energy[r] = saved_energy[r];
        return;
    }
    if (!(energy[r] < best_energy[r])) return;
    const int4 *src = reinterpret_cast<const int4 *>(spins + (long long)r * sstride);
    int4 *dst = reinterpret_cast<int4 *>(best_spins + (long long)r * sstride);
    for (int i = threadIdx.x; i < sstride / 16; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
    if (threadIdx.x == 0) best_energy[r] = energy[r];
}

hipError_t launch_cluster_moves(const ClusterArgs &a, hipStream_t st) {
    if (a.count <= 0) return hipSuccess;
    const size_t lds = cluster_lds_bytes(a.n);
    if (a.n <= 0 || lds > CLUSTER_LDS_BUDGET || a.sstride % 16 != 0 || a.sstride < a.n) return hipErrorInvalidValue;
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(cluster_moves_kernel), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cluster_moves_kernel, dim3(a.count), dim3(CLUSTER_THREADS), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_cluster_finish(const int *touched, const double *saved_energy, double *energy, const int8_t *spins,
                                 double *best_energy, int8_t *best_spins, int sstride, int R, hipStream_t st) {
    hipLaunchKernelGGL(cluster_finish_kernel, dim3(R), dim3(256), 0, st, touched, saved_energy, energy, spins, best_energy,
                       best_spins, sstride, R);
    return hipGetLastError();
}

}  // namespace sga
