// worldline_clusters.hip -- simulated quantum annealing: Swendsen-Wang clusters along imaginary time at one site, flipped
// under the classical field (sga_worldline_clusters).
//
// The local replicas are G groups of P Trotter slices, as in sweep_transverse.hip.  One launch serves all n_sweeps of a
// call: one workgroup of ONE WAVE per group, lane p = slice p, and nothing is shared between workgroups.  It is the first
// kernel here in which the replicas of a group act together inside one update: a coupling row is read once for all P
// slices of a site.
//
// Spins: one word per site in LDS, bit p = [s_p[i] < 0] (uint32_t for P <= 32, uint64_t beyond), transposed in from the
// int8 rows at entry and written back -- with any new bests -- from LDS.
// Rows: typewriter order makes rowptr64 / cv one forward stream.  The wave holds a window of 64 entries of cv, one per
// lane, and the 64 behind them, requested a window ahead of the site being decided; an entry is handed to every lane by
// v_readlane, every lane reads the SAME LDS word (a broadcast) and takes its own bit.  The extent and the field of the
// next site are requested while this one is decided.
// Segments: the active bonds are one ballot; heads, the head of a lane and a segment's size are bit arithmetic on that
// mask, the wrap through slice 0 included.  The segmented integer sums go through LDS integer atomics: every lane adds
// its row sum to the accumulator of its head (ds_add_u32), every lane then takes and clears its own accumulator
// (ds_wrxchg_rtn_b32) -- two LDS operations, against six DPP steps and two ds_bpermute of a prefix scan with the wrap
// patched in.
// The decision is the oracle's fp64 Metropolis rule on Phi = A + m h_i, taken on the head's lane with the head's uniform.
// No load under a lane condition (lanes >= P run along on clamped indices and add zeros), no scratch.
#include "sga_quantum.h"
#include "sweep_common.h"

namespace sga {

namespace {

template <typename Word>
__device__ __forceinline__ uint32_t bit_of(Word w, int p) {
    if constexpr (sizeof(Word) == 4)
        return (w >> (p & 31)) & 1u;  // (lanes >= 32 mirror the lower half; they are masked by p < P)
    else
        return (uint32_t)(w >> p) & 1u;
}

// int8 spins of 4 consecutive sites of slice p (+-1, pad = 0) out of the 4 words
template <typename Word>
__device__ __forceinline__ uint32_t spin_dword(const Word (&w)[4], int p, int site0, int n) {
    uint32_t d = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) d |= (site0 + q < n ? (bit_of(w[q], p) ? 0xFFu : 0x01u) : 0u) << (8 * q);
    return d;
}

template <typename Word>
__global__ void __launch_bounds__(64) worldline_clusters_kernel(const SweepArgs a, const WorldlineArgs q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const int g = (int)blockIdx.x;
    const int P = q.n_slices, n = a.n;
    const int G = a.R / P;
    const int n4 = (n + 3) >> 2;  // dwords of int8 spins that hold a site
    Word *s = reinterpret_cast<Word *>(smem);
    int *acc = reinterpret_cast<int *>(smem + (size_t)n4 * 4 * sizeof(Word));
    const bool mine = lane < P;
    const int p = mine ? lane : P - 1;  // lanes >= P run along on slice P - 1 and store nothing
    const int r = slice_row(g, P, p);
    const int pn = ring_next(p, P);
    const unsigned long long ring = P == 64 ? ~0ull : (1ull << P) - 1ull;

    // the int8 rows -> words, 4 sites (one dword of each row) a step
    for (int c = lane; c < n4; c += 64) {
        Word w[4] = {0, 0, 0, 0};
        for (int pp = 0; pp < P; ++pp) {
            const uint32_t d = reinterpret_cast<const uint32_t *>(a.spins + (long long)slice_row(g, P, pp) * a.sstride)[c];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] |= (Word)((d >> (8 * k + 7)) & 1u) << pp;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s[4 * c + k] = w[k];
    }
    acc[lane] = 0;
    __builtin_amdgcn_wave_barrier();

    auto sload_ll = [&](const long long *x) -> long long { return *(const __attribute__((address_space(4))) long long *)x; };
    auto sload_f = [&](const float *x) -> float { return *(const __attribute__((address_space(4))) float *)x; };
    const double T = a.rep_temp[g * P];
    double E = a.energy[r], bestE = a.best_energy[r];
    const long long nnz = sload_ll(a.rowptr64 + n);
    long long n_seg = 0, n_segflip = 0, n_spinflip = 0;

    // the window of cv: entries [wbase, wbase + 64) in (col, val), the next 64 in (col2, val2); past the array's end a
    // lane holds the last entry again (a clamped index, no condition on the load) and is never handed out
    auto load_window = [&](long long base, int &col, int &val) {
        if (nnz > 0) {  // wave-uniform
            const long long at = base + lane < nnz ? base + lane : nnz - 1;
            const int2 ent = a.cv[at];
            col = ent.x;
            val = (int)__int_as_float(ent.y);  // integer couplings: exact
        }
    };

    for (int kk = 0; kk < q.n_sweeps; ++kk) {
        const uint32_t thr = *(const __attribute__((address_space(4))) uint32_t *)(q.thr + (size_t)kk * G + g);
        long long beg = sload_ll(a.rowptr64);
        long long wbase = beg;
        int col = 0, val = 0, col2 = 0, val2 = 0;
        load_window(wbase, col, val);
        load_window(wbase + 64, col2, val2);
        long long end = sload_ll(a.rowptr64 + 1);
        float h = sload_f(a.h);
        for (int i = 0; i < n; ++i) {
            // the next site's extent and field, requested now
            const int nx = i + 1 < n ? i + 1 : i;
            const long long end_nx = sload_ll(a.rowptr64 + nx + 1);
            const float h_nx = sload_f(a.h + nx);
            // the draws do not depend on the spins.  (Computed a site ahead instead, beside the segment logic of the site
            // before it, a sweep took 13.07 against 13.10 ms on the 22^3 lattice and 28.6 against 29.0 on C3: not kept.)
            const u32x4 rnd = worldline_block((uint32_t)i, q.round + (uint32_t)kk, a.replica0 + (uint32_t)r, a.seed_lo, a.seed_hi);
            const Word word = s[i];
            // dot_p = sum_j J_ij s_p[j]
            int dot = 0;
            for (long long e = beg; e < end;) {
                if (e - wbase >= 64) {  // the window moves on, the one behind it is requested
                    wbase += 64;
                    col = col2, val = val2;
                    load_window(wbase + 64, col2, val2);
                }
                const int k0 = (int)(e - wbase);
                const int cnt = (int)(end - e) < 64 - k0 ? (int)(end - e) : 64 - k0;
                // four entries a step, their LDS reads in flight together (the compiler does not unroll a loop of
                // v_readlane); a step past the run's end hands out the window's last lanes with the value 0
                for (int k = 0; k < cnt; k += 4) {
                    Word wj[4];
                    int v[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int at = k0 + k + t < 63 ? k0 + k + t : 63;
                        wj[t] = s[__builtin_amdgcn_readlane(col, at)];
                        v[t] = k + t < cnt ? __builtin_amdgcn_readlane(val, at) : 0;
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t) dot += bit_of(wj[t], p) ? -v[t] : v[t];
                }
                e += cnt;
            }
            // bonds, heads, segments
            const uint32_t sb = bit_of(word, p);
            const bool bond = mine && sb == bit_of(word, pn) && (rnd.x >> 8) < thr;
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
            s[i] = word ^ (Word)flips;  // every lane the same value
            if (my_flip) E += 2.0 * sigma * ((double)dot + (double)h);
            n_seg += __builtin_popcountll(heads);
            n_segflip += __builtin_popcountll(flipped_heads);
            n_spinflip += __builtin_popcountll(flips);
            beg = end, end = end_nx, h = h_nx;
        }
        // the sweep's end: the best follows where the energy is lower
        const bool lower = mine && E < bestE;
        if (lower) bestE = E;
        unsigned long long todo = ballot64(lower);
        while (todo) {  // wave-uniform
            const int pp = __builtin_ctzll(todo);
            todo &= todo - 1;
            uint32_t *dst = reinterpret_cast<uint32_t *>(a.best_spins + (long long)slice_row(g, P, pp) * a.sstride);
            for (int c = lane; c < n4; c += 64) {
                const Word w[4] = {s[4 * c], s[4 * c + 1], s[4 * c + 2], s[4 * c + 3]};
                dst[c] = spin_dword(w, pp, 4 * c, n);
            }
        }
    }

    for (int c = lane; c < n4; c += 64) {
        const Word w[4] = {s[4 * c], s[4 * c + 1], s[4 * c + 2], s[4 * c + 3]};
        for (int pp = 0; pp < P; ++pp)
            reinterpret_cast<uint32_t *>(a.spins + (long long)slice_row(g, P, pp) * a.sstride)[c] = spin_dword(w, pp, 4 * c, n);
    }
    if (mine) {
        a.energy[r] = E;
        a.best_energy[r] = bestE;
    }
    if (q.stats && lane < 3) q.stats[3 * g + lane] = lane == 0 ? n_seg : lane == 1 ? n_segflip : n_spinflip;
}

}  // namespace

hipError_t launch_worldline_clusters(const SweepArgs &a, const WorldlineArgs &w, hipStream_t st) {
    if (!a.rowptr64 || !a.cv || !a.h || !a.spins || !a.best_spins || !a.energy || !a.best_energy || !a.rep_temp || !w.thr ||
        w.n_slices < 2 || w.n_slices > WORLDLINE_MAX_SLICES || a.R % w.n_slices != 0 || a.replica0 % (uint32_t)w.n_slices != 0 ||
        w.n_sweeps < 1 || a.sstride % 16 != 0 || a.n > worldline_max_sites(w.n_slices))
        return hipErrorInvalidValue;
    const size_t lds = worldline_lds_bytes(a.n, w.n_slices);
    const bool wide = worldline_word_bytes(w.n_slices) == 8;
    const auto kern = wide ? worldline_clusters_kernel<uint64_t> : worldline_clusters_kernel<uint32_t>;
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(a.R / w.n_slices), dim3(64), lds, st, a, w);
    note_sweep_kernel("worldline_clusters_kernel<%d-bit words, %d slices> x %d sweep(s)", wide ? 64 : 32, w.n_slices, w.n_sweeps);
    return hipGetLastError();
}

}  // namespace sga
