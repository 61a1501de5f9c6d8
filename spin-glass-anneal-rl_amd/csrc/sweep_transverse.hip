// sweep_transverse.hip -- simulated quantum annealing: the Trotter slices of one instance coupled in the CSR sweep
// (sga_sweep_transverse).
//
// The local replicas are G groups of P slices.  One launch is one HALF-SWEEP: the slices of one parity move, each through
// the n updates of sga_sweep's production stream (Philox block t >> 1 of (sweep, global replica), domain 0), the slices
// of the other parity stand still.  P is even, so both neighbours p +- 1 of a moving slice stand still: their int8 rows
// in HBM are read-only for the whole launch, and the kernel boundary is the only synchronisation between slices -- no
// workgroup waits on, signals or reads anything another workgroup writes.
//
// The form is the narrow one-update CSR form's (sweep_csr_impl.h): one wave per moving slice, the slice's spins as int8
// in a private LDS range, no workgroup barrier, the row of a proposal gathered by the wave (64 entries a load, longer
// rows in further loads), the dot a DPP wave sum in fp32 -- exact in any order for the classes the call admits.  What is
// indexed by the site alone -- the row's extent, h, the diagonal and the two neighbour spins -- is requested a pair of updates
// ahead, the row's first 64 entries one update ahead, while the update before it is reduced.
//
// The decision is metropolis_accept on h_eff = h_i + k (s_up[i] + s_dn[i]); the tracked energy moves by the classical dE,
// the same expression with h_i.
//
// An accept table for the proposals whose h_eff is exact (h_i = 0 or a = 0: thresholds per (s_i a / 2, integer s_i (dot +
// h_i)) tabulated per launch in LDS) was built, held against the reference and measured: 8.69 against 8.56 ms per sweep
// on the 22^3 lattice, 8.51 against 8.22 on C3's graph -- slower, its index arithmetic and 12 spilled SGPRs costing more than
// the divide and the exp of the uphill proposals.  Every proposal takes metropolis_accept.
//
// A pre-kernel variant (build macro SGA_TRANSVERSE_PREPASS) was measured and then removed: instead of the two neighbour
// bytes, a kernel before each half-sweep wrote h_eff[r][i] for the moving slices and the sweep gathered one float.  Level
// with the byte loads on the 22^3 lattice (8.54 against 8.56 ms per sweep) and slower on C3's graph (8.99 against 8.22), at
// R n floats of scratch and a third launch per half-sweep.  The figures are kept in DESIGN.md 4.9 and under "variants" in
// profiles/transverse.json.
#include "sga_quantum.h"
#include "sweep_common.h"

namespace sga {

namespace {

// dE of the rule for a flip of s_i under field h_site, as metropolis_accept forms it (Metropolis rule)
__device__ __forceinline__ double rule_dE(int arith, float dot, int si, float h_site, float diag_site) {
    if (arith == SGA_ARITH_F64) return 2.0 * (double)si * ((double)dot + (double)h_site);
    const float sif = (float)si;
    const float field = (h_site + dot) - diag_site * sif;
    return (double)((2.0f * sif) * field);
}

template <bool F32>  // SGA_ARITH_F32 (the rule in fp32, J_ii subtracted)
__global__ void __launch_bounds__(64 * CSR_WAVES_PER_BLOCK) sweep_transverse_kernel(const SweepArgs a, const TrotterLaunch q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nw = blockDim.x >> 6;
    const int m = (int)blockIdx.x * nw + w;  // moving slice of this wave
    if (m >= q.moving) return;               // wave-uniform; no barriers
    const MovingSlice sl = moving_slice(m, q.n_slices, q.parity);
    const int r = sl.r;
    const int8_t *up = a.spins + (long long)sl.up * a.sstride;
    const int8_t *dn = a.spins + (long long)sl.dn * a.sstride;
    const float kp = *(const __attribute__((address_space(4))) float *)(q.k_perp + sl.g);
    const int n = a.n;
    constexpr int arith = F32 ? SGA_ARITH_F32 : SGA_ARITH_F64;
    constexpr bool arith32 = F32;
    int8_t *s = reinterpret_cast<int8_t *>(smem) + (long long)w * a.sstride;
    {
        const int4 *src = reinterpret_cast<const int4 *>(a.spins + (long long)r * a.sstride);
        int4 *dst = reinterpret_cast<int4 *>(s);
        for (int i = lane; i < a.sstride / 16; i += 64) dst[i] = src[i];
    }
    // set-time arrays, indexed by the wave-uniform site: through the scalar data cache
    auto sload_ll = [&](const long long *x) -> long long { return *(const __attribute__((address_space(4))) long long *)x; };
    auto sload_f = [&](const float *x) -> float { return *(const __attribute__((address_space(4))) float *)x; };
    const double T = a.rep_temp[r];
    double E = a.energy[r];
    unsigned long long nacc = 0;

    struct Extent {  // what is indexed by the site alone: requested a PAIR of updates ahead
        long long beg;
        int len;
        float h, d;
        int nb;  // s_up[site] + s_dn[site]
    };
    struct Head {  // the row's first 64 entries, one per lane: requested one update ahead, once the extent is back
        const int2 *row;
        int2 ent;
    };
    auto load_extent = [&](int site) {
        Extent o;
        const int us = __builtin_amdgcn_readfirstlane(site);
        o.beg = sload_ll(a.rowptr64 + us);
        o.len = (int)(sload_ll(a.rowptr64 + us + 1) - o.beg);
        o.h = sload_f(a.h + us);
        o.d = arith32 ? sload_f(a.diag + us) : 0.0f;
        o.nb = (int)up[us] + (int)dn[us];
        return o;
    };
    auto load_head = [&](const Extent &x) {
        Head o;
        o.row = a.cv + x.beg;
        // (no bounds test: lanes past the row's end hold entries of the rows behind it, or of the zeroed entries that
        // follow the array, and are masked when the row is summed)
        o.ent = o.row[lane];
        return o;
    };
    auto update = [&](int site, float u, const Extent &x, const Head &hd) {
        const int si = s[site];
        float acc = (lane < x.len ? __int_as_float(hd.ent.y) : 0.0f) * (float)s[hd.ent.x];
        for (int c0 = 64; c0 < x.len; c0 += 64) {  // rows beyond 64 entries
            const int2 ent = hd.row[c0 + lane];
            acc += (lane < x.len - c0 ? __int_as_float(ent.y) : 0.0f) * (float)s[ent.x];
        }
        const float dot = wave_sum(acc);
        const float h_eff = x.h + kp * (float)x.nb;  // the product is exact: one rounding
        double dE_eff;
        const bool flip = metropolis_accept(SGA_RULE_METROPOLIS, arith, dot, si, h_eff, x.d, T, u, dE_eff);
        if (flip) {
            E += rule_dE(arith, dot, si, x.h, x.d);  // the slice's classical energy -1/2 s J s - h s
            ++nacc;
            if (lane == 0) s[site] = (int8_t)(-si);
        }
    };

    // Pairs of updates (one Philox block each), as the narrow CSR form walks them: the extents of the next pair and the
    // head of its first row are requested while this pair is reduced, so no update waits on an extent -> entry chain of two
    // memory round trips (with both requested one update ahead a sweep of the 22^3 lattice took 10.5 ms, not 9.7).  Two
    // sets of variables swap roles instead of being rotated.
    struct PairState {
        UpdatePair p;
        Extent xA, xB;
        Head hA;
    };
    PairSource<true> rng;
    const int nb = (n + 1) >> 1;
    PairState S0, S1;
    S0.p = rng.get(a, r, 0, 0, true, lane);
    S0.xA = load_extent(S0.p.sA);
    S0.xB = load_extent(S0.p.sB);
    S0.hA = load_head(S0.xA);
    auto pair = [&](PairState &c, PairState &nx, int b) {
        nx.p = rng.get(a, r, 0, b + 1, b + 1 < nb, lane);  // past the end: site 0
        const bool hasB = (2 * b + 1) < n;
        nx.xA = load_extent(nx.p.sA);  // a pair ahead
        nx.xB = load_extent(nx.p.sB);
        Head hB{};
        if (hasB) hB = load_head(c.xB);  // in flight while A is reduced
        update(c.p.sA, c.p.uA, c.xA, c.hA);
        nx.hA = load_head(nx.xA);        // in flight while B is reduced
        if (hasB) update(c.p.sB, c.p.uB, c.xB, hB);
    };
    {
        int b = 0;
        for (; b + 1 < nb; b += 2) {
            pair(S0, S1, b);
            pair(S1, S0, b + 1);
        }
        if (b < nb) pair(S0, S1, b);
    }

    {
        int4 *dst = reinterpret_cast<int4 *>(a.spins + (long long)r * a.sstride);
        const int4 *src = reinterpret_cast<const int4 *>(s);
        for (int i = lane; i < a.sstride / 16; i += 64) dst[i] = src[i];
    }
    // the slice moved in this half-sweep only: its energy now is its energy at the sweep's end, where the best follows
    double bestE = a.best_energy[r];
    if (E < bestE) {
        bestE = E;
        int4 *dst = reinterpret_cast<int4 *>(a.best_spins + (long long)r * a.sstride);
        const int4 *src = reinterpret_cast<const int4 *>(s);
        for (int i = lane; i < a.sstride / 16; i += 64) dst[i] = src[i];
    }
    if (lane == 0) {
        a.energy[r] = E;
        a.best_energy[r] = bestE;
        a.n_accepted[r] += nacc;
    }
}

}  // namespace

hipError_t launch_sweep_transverse(const SweepArgs &a, const TrotterLaunch &t, hipStream_t st) {
    const int waves = transverse_waves_per_block(a.sstride);
    if (waves < 1 || !a.rowptr64 || !a.cv || !a.h || !a.spins || !t.k_perp || t.n_slices < 2 || (t.n_slices & 1) ||
        a.R % t.n_slices != 0 || t.moving != a.R / 2 || a.sstride % 16 != 0 || (a.arith == SGA_ARITH_F32 && !a.diag))
        return hipErrorInvalidValue;
    const size_t lds = (size_t)waves * (size_t)a.sstride;
    // (built per arithmetic: with a run-time arith both rules' code and scalars stay live -- 9.70 against 8.56 ms per sweep
    // on the 22^3 lattice)
    const auto kern = a.arith == SGA_ARITH_F32 ? sweep_transverse_kernel<true> : sweep_transverse_kernel<false>;
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((t.moving + waves - 1) / waves), dim3(64 * waves), lds, st, a, t);
    note_sweep_kernel("sweep_transverse_kernel<%s, %d slices, parity %d> x %d slice(s) per workgroup",
                      a.arith == SGA_ARITH_F32 ? "f32 rule" : "f64 rule", t.n_slices, t.parity, waves);
    return hipGetLastError();
}

}  // namespace sga
