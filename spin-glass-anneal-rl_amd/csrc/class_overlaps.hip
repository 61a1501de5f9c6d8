// class_overlaps.hip -- the overlap between two replicas resolved by a class of sites, measured where the spins are:
// sga_get_class_overlaps / sga_accumulate_ladder_class_overlaps.
//
// A class map gives every site a class in [0, C) -- the planes of a lattice, sublattices, communities -- or none (any
// value outside the range).  For a pair (a, b) with x_i = [s_a[i] != s_b[i]] and a map m:
// D[m][c] = sum_{i : classes[m][i] = c} x_i, so that the class overlap is Q_c = N_c - 2 D_c.  Everything is an integer
// count: the result does not depend on any order.
//
// Mapping: one workgroup of 256 threads per pair (the pair and slot lookup of pair_overlaps_kernel).  1. a lane takes
// four consecutive sites, a wave 256 a step: one dword of each spin row and one int4 of each map a lane (scalar words
// where the caller's map is not 16-byte aligned), class words only in the waves and lanes that differ; a differing
// site whose class is in range adds 1 to cnt[m C + c] in LDS.  Every wave has a copy of the counters of its own where four fit (class_overlap_copies), and where a ballot shows that the wave's
// in-range lanes share one class -- every map but the fastest axis's on a row-major lattice -- one lane adds the
// popcount.  2. the copies are summed; the pair form stores D, the ladder form adds D to the cell's sum1 and, asked
// for, D[m][c] D[m][c'] to its sum2, the threads striding over the entries (one workgroup owns one cell per launch: a
// plain 64-bit load / add / store).  No loop depends on the data: n sites, M maps, M C and M C^2 entries.
#include "sweep_common.h"

#ifndef SGA_CLASS_OVERLAP_SHORTCUT  // (a measurement build passes 0: profiles/class_overlaps_timing.py)
#define SGA_CLASS_OVERLAP_SHORTCUT 1
#endif

namespace sga {

__global__ void __launch_bounds__(CLASS_OVERLAP_THREADS) class_overlaps_kernel(const ClassOverlapArgs a, const int copies) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned int *cnt = reinterpret_cast<unsigned int *>(smem);  // [copies][M C]
    const int n = a.n, M = a.n_maps, C = a.n_classes, MC = M * C;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = blockIdx.x;

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

    for (int k = tid; k < copies * MC; k += CLASS_OVERLAP_THREADS) cnt[k] = 0u;
    __syncthreads();

    // 1. the walk: a lane takes four consecutive sites a step (one dword of each spin row, one int4 of each map), a
    // wave 256; the steps are the same for every lane of a wave, so the ballots see whole waves
    unsigned int *mine = cnt + (copies == 4 ? wave * MC : 0);
    for (int base = wave * 256; base < n; base += 4 * CLASS_OVERLAP_THREADS) {
        const int i0 = base + 4 * lane;
        unsigned int x = 0u;  // bit j: site i0 + j differs
        if (i0 < n) {         // (rows end at a multiple of 16: the dword lies inside the row)
            const unsigned int d = *reinterpret_cast<const unsigned int *>(sa + i0) ^ *reinterpret_cast<const unsigned int *>(sb + i0);
            x = ((d & 0xffu) ? 1u : 0u) | ((d & 0xff00u) ? 2u : 0u) | ((d & 0xff0000u) ? 4u : 0u) | ((d & 0xff000000u) ? 8u : 0u);
            if (n - i0 < 4) x &= (1u << (n - i0)) - 1u;  // the pad past n is no site
        }
        if (__ballot(x != 0u) == 0ull) continue;
        for (int m = 0; m < M; ++m) {
            const int32_t *row = a.classes + (long long)m * a.ld + i0;
            int c4[4] = {-1, -1, -1, -1};
            if (x != 0u) {
                if (a.vec_classes && i0 + 4 <= n) {  // 16-byte aligned rows, and all four words are sites of the row
                    const int4 v = *reinterpret_cast<const int4 *>(row);
                    c4[0] = v.x, c4[1] = v.y, c4[2] = v.z, c4[3] = v.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((x >> j) & 1u) c4[j] = row[j];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c4[j];
                const bool in = ((x >> j) & 1u) && (unsigned int)c < (unsigned int)C;  // the range is tested, never trusted
                const unsigned long long mask = __ballot(in);
                if (mask == 0ull) continue;
#if SGA_CLASS_OVERLAP_SHORTCUT
                const int first = __ffsll(mask) - 1;
                const int c0 = __builtin_amdgcn_readlane(c, first);  // (first is the same in every lane: a scalar read)
                if (__ballot(in && c != c0) == 0ull) {  // one class in the whole wave
                    if (lane == first) atomicAdd(&mine[m * C + c0], (unsigned int)__popcll(mask));
                    continue;
                }
#endif
                if (in) atomicAdd(&mine[m * C + c], 1u);
            }
        }
    }
    __syncthreads();

    // 2. the copies summed
    for (int k = tid; k < MC; k += CLASS_OVERLAP_THREADS) {
        unsigned int v = cnt[k];
        if (copies == 4) v += cnt[MC + k] + cnt[2 * MC + k] + cnt[3 * MC + k];
        if (a.pairs) {
            a.dist[(size_t)p * (size_t)MC + k] = (int32_t)v;
        } else {
            a.sum1[(size_t)p * (size_t)MC + k] += (unsigned long long)v;
            cnt[k] = v;
        }
    }
    if (a.pairs || !a.sum2) return;
    __syncthreads();
    // entry (m C + c) C + c' of the cell: M C^2 <= 40 896^2 < 2^32
    unsigned long long *s2 = a.sum2 + (size_t)p * (size_t)MC * (size_t)C;
    const unsigned int entries = (unsigned int)MC * (unsigned int)C;
    for (unsigned int idx = tid; idx < entries; idx += CLASS_OVERLAP_THREADS) {
        const unsigned int row = idx / (unsigned int)C, c2 = idx - row * (unsigned int)C, m = row / (unsigned int)C;
        s2[idx] += (unsigned long long)cnt[row] * (unsigned long long)cnt[m * (unsigned int)C + c2];
    }
}

hipError_t launch_class_overlaps(const ClassOverlapArgs &a, hipStream_t st) {
    if (a.count <= 0) return hipSuccess;
    const long long mc = (long long)a.n_maps * (long long)a.n_classes;
    if (a.n <= 0 || a.n_maps < 1 || a.n_classes < 1 || mc > CLASS_OVERLAP_MAX_MC || a.ld < a.n || a.sstride < a.n || a.sstride % 4 != 0 || !a.classes ||
        (a.pairs ? !a.dist : (!a.sum1 || !a.slot_to_rep || a.n_slots < 1)))
        return hipErrorInvalidValue;
    const size_t lds = class_overlap_lds_bytes(mc);
    ClassOverlapArgs b = a;
    b.vec_classes = reinterpret_cast<uintptr_t>(a.classes) % 16 == 0 && a.ld % 4 == 0 ? 1 : 0;
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(class_overlaps_kernel), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(class_overlaps_kernel, dim3(a.count), dim3(CLASS_OVERLAP_THREADS), lds, st, b, class_overlap_copies(mc));
    return hipGetLastError();
}

}  // namespace sga
