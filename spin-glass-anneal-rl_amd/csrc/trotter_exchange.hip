// trotter_exchange.hip -- the broken time links of every Trotter group, and one round of replica exchange between
// neighbouring groups along the transverse field (sga_get_time_links, sga_exchange_transverse).
//
// B_g = sum_p sum_i [ s_{gP+p}[i] != s_{gP+ring_next(p)}[i] ] is all of a configuration that the quantum estimators and the
// acceptance ratio of an exchange along Gamma read (the rule: include/sga.h).
//
// time_links_kernel, the one that reads every spin byte: a grid of (site chunks x groups), one wave per workgroup, a lane
// holding 16 consecutive sites.  The wave walks p = 0 ... P - 1 with the previous slice's 16 bytes in registers and slice
// 0's kept for the wrap, so a byte is loaded once.  Spins are +-1 (0x01 | 0xFF) with a zero pad: a ^ b is 0x00 or 0xFE per
// byte, bit 7 of each byte counts.  A wave sum, then one 64-bit integer atomic per workgroup: exact in any order.  A lane
// past the row's end loads at a clamped index and counts nothing: no load under a lane condition.
//
// The exchange is three launches on one stream: the counts, trotter_exchange_decide_kernel (the only reader of B and the
// energies, one thread per group, both groups of a pair deciding alike) and trotter_exchange_swap_kernel over (chunk,
// slice, pair), 16 bytes a lane of the spin rows and, where they are valid, of the resident field rows; one lane trades
// the tracked energies as bits.  The swap overwrites the energies the decision reads: they do not share a launch.
#include <algorithm>

#include "sga_quantum.h"
#include "sweep_common.h"

namespace sga {

namespace {

constexpr int SWAP_THREADS = 256;

__device__ __forceinline__ int differing_bytes(const int4 &a, const int4 &b) {
    return __builtin_popcount((uint32_t)(a.x ^ b.x) & 0x80808080u) + __builtin_popcount((uint32_t)(a.y ^ b.y) & 0x80808080u) +
           __builtin_popcount((uint32_t)(a.z ^ b.z) & 0x80808080u) + __builtin_popcount((uint32_t)(a.w ^ b.w) & 0x80808080u);
}

__global__ void __launch_bounds__(64) time_links_kernel(const int8_t *spins, int sstride, int P, long long *links) {
    const int lane = (int)threadIdx.x;
    const int g = (int)blockIdx.y;
    const int c = (int)blockIdx.x * 64 + lane;  // the lane's 16 bytes of every row
    const bool inside = c < sstride / 16;
    const int4 *row = reinterpret_cast<const int4 *>(spins + (long long)slice_row(g, P, 0) * sstride) + (inside ? c : 0);
    const int step = sstride / 16;
    const int4 first = row[0];
    int4 prev = first;
    int count = 0;
#pragma unroll 4
    for (int p = 1; p < P; ++p) {
        const int4 cur = row[(long long)p * step];
        count += differing_bytes(prev, cur);
        prev = cur;
    }
    count += differing_bytes(prev, first);  // the wrap (P = 2: the one link a second time, as the sweep counts it)
    const int total = wave_sum(inside ? count : 0);
    if (lane == 0 && total != 0) atomicAdd(reinterpret_cast<unsigned long long *>(links) + g, (unsigned long long)total);
}

// Thread g decides the pair its group stands in, if any, and writes flags[g]; every operation a single fp64 one.
__global__ void trotter_exchange_decide_kernel(const SweepArgs s, const TrotterExchangeArgs x) {
    const int P = x.n_slices, G = s.R / P;
    const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (g >= G) return;
    const int a = (g & 1) == x.parity ? g : g - 1, b = a + 1;
    int flag = 0;
    if (a >= 0 && b < G) {
        const double Ta = s.rep_temp[slice_row(a, P, 0)], Tb = s.rep_temp[slice_row(b, P, 0)];
        const bool usable = Ta > 0.0 && Ta < __builtin_inf() && Tb > 0.0 && Tb < __builtin_inf();
        if (usable) {
            const double beta_a = 1.0 / Ta, beta_b = 1.0 / Tb;
            double Ea = s.energy[slice_row(a, P, 0)], Eb = s.energy[slice_row(b, P, 0)];
            for (int p = 1; p < P; ++p) {
                Ea += s.energy[slice_row(a, P, p)];
                Eb += s.energy[slice_row(b, P, p)];
            }
            const double t1 = (beta_a - beta_b) * (Ea - Eb);
            const double c = beta_a * (double)x.k_perp[a] - beta_b * (double)x.k_perp[b];
            const double t2 = (2.0 * c) * (double)(x.links[a] - x.links[b]);
            const double xx = t1 + t2;
            const double prob = !(xx < 0.0) ? 1.0 : exp_det(xx);
            const double u = trotter_exchange_u(x.round, (uint32_t)a, s.seed_lo, s.seed_hi);
            flag = u < prob ? 1 : 0;
        }
    }
    x.flags[g] = flag;
}

__device__ __forceinline__ void trade16(int4 *pa, int4 *pb) {
    const int4 va = *pa, vb = *pb;
    *pa = vb;
    *pb = va;
}

// blockIdx: (chunk of SWAP_THREADS x 16 bytes, slice p, pair).  The flag is uniform per workgroup.
__global__ void __launch_bounds__(SWAP_THREADS) trotter_exchange_swap_kernel(const SweepArgs s, const TrotterExchangeArgs x) {
    const int P = x.n_slices;
    const int a = x.parity + 2 * (int)blockIdx.z;
    if (!x.flags[a]) return;
    const int ra = slice_row(a, P, (int)blockIdx.y), rb = slice_row(a + 1, P, (int)blockIdx.y);
    const long long idx = (long long)blockIdx.x * SWAP_THREADS + threadIdx.x;
    if (idx < s.sstride / 16)
        trade16(reinterpret_cast<int4 *>(s.spins + (long long)ra * s.sstride) + idx, reinterpret_cast<int4 *>(s.spins + (long long)rb * s.sstride) + idx);
    if (x.fields && idx < x.field_row_bytes / 16) {
        unsigned char *F = static_cast<unsigned char *>(x.fields);
        trade16(reinterpret_cast<int4 *>(F + (long long)ra * x.field_row_bytes) + idx, reinterpret_cast<int4 *>(F + (long long)rb * x.field_row_bytes) + idx);
    }
    if (idx == 0) {  // the tracked energies, as bits
        unsigned long long *E = reinterpret_cast<unsigned long long *>(s.energy);
        const unsigned long long ea = E[ra], eb = E[rb];
        E[ra] = eb;
        E[rb] = ea;
    }
}

}  // namespace

hipError_t launch_time_links(const int8_t *spins, int sstride, int R, int n_slices, long long *links, hipStream_t st) {
    if (!spins || !links || sstride < 16 || sstride % 16 != 0 || n_slices < 2 || R < n_slices || R % n_slices != 0 ||
        R / n_slices > 65535)  // (the groups are the grid's second dimension)
        return hipErrorInvalidValue;
    const int chunks = (sstride + TIME_LINKS_CHUNK_SITES - 1) / TIME_LINKS_CHUNK_SITES;
    hipLaunchKernelGGL(time_links_kernel, dim3(chunks, R / n_slices), dim3(64), 0, st, spins, sstride, n_slices, links);
    note_sweep_kernel("time_links_kernel<%d slices> x %d chunk(s) x %d group(s)", n_slices, chunks, R / n_slices);
    return hipGetLastError();
}

namespace {
bool exchange_args_ok(const SweepArgs &a, const TrotterExchangeArgs &x) {
    return a.spins && a.energy && a.rep_temp && x.k_perp && x.links && x.flags && a.sstride >= 16 && a.sstride % 16 == 0 &&
           x.n_slices >= 2 && x.n_slices <= 65535 && a.R / x.n_slices <= 2 * 65535 && a.R >= x.n_slices && a.R % x.n_slices == 0 && (x.parity == 0 || x.parity == 1) &&
           (!x.fields || (x.field_row_bytes > 0 && x.field_row_bytes % 16 == 0));
}
}  // namespace

hipError_t launch_trotter_exchange_decide(const SweepArgs &a, const TrotterExchangeArgs &x, hipStream_t st) {
    if (!exchange_args_ok(a, x)) return hipErrorInvalidValue;
    const int G = a.R / x.n_slices;
    hipLaunchKernelGGL(trotter_exchange_decide_kernel, dim3((G + 63) / 64), dim3(64), 0, st, a, x);
    return hipGetLastError();
}

hipError_t launch_trotter_exchange_swap(const SweepArgs &a, const TrotterExchangeArgs &x, hipStream_t st) {
    if (!exchange_args_ok(a, x)) return hipErrorInvalidValue;
    const int G = a.R / x.n_slices;
    const int pairs = (G - x.parity) / 2;  // a = parity, parity + 2, ... with a + 1 < G
    note_sweep_kernel("trotter_exchange_kernel<%d slices, fields %s> x %d pair(s)", x.n_slices, x.fields ? "traded" : "left alone", pairs);
    if (pairs < 1) return hipSuccess;
    const long long units = std::max<long long>(a.sstride / 16, x.fields ? x.field_row_bytes / 16 : 0);
    const unsigned chunks = (unsigned)((units + SWAP_THREADS - 1) / SWAP_THREADS);
    hipLaunchKernelGGL(trotter_exchange_swap_kernel, dim3(chunks, x.n_slices, pairs), dim3(SWAP_THREADS), 0, st, a, x);
    return hipGetLastError();
}

}  // namespace sga
