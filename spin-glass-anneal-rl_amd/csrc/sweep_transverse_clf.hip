// sweep_transverse_clf.hip -- simulated quantum annealing on DENSE couplings, carried by the cached local fields
// (sga_sweep_transverse_dense).
//
// The step is sga_sweep_transverse's (sweep_transverse.hip), the form is the cached-local-field sweep's (sweep_clf_impl.h).
// The local replicas are G groups of P slices; one launch is one HALF-SWEEP: the slices of one parity move, each through
// the n updates of sga_sweep's production stream, the slices of the other parity stand still.  P is even, so both
// neighbours of a moving slice stand still: a_i = s_up[i] + s_dn[i] is a constant of the launch, and the resident fields
// F = scale (J s + h) of the moving slice do not contain it.  The decision of a candidate is a pure function of (F_i, s_i,
// a_i, u) and a rejected proposal leaves the state untouched -- the window logic of sweep_clf_kernel carries over as it
// stands: 128 updates per wave evaluated at once, the first accept applied (row i of J read once), the candidates behind
// it evaluated again.
//
// One workgroup per moving slice, W waves.  LDS: the slice's fields | its spins as bits | the two neighbour slices' spins
// as bits (n / 4 bytes, staged once per launch with coalesced 16-byte loads from their int8 rows) | the decision slots.
// What depends on a candidate's SITE alone is formed once per super-window and kept in registers: h_i (gathered from the
// 4 n-byte vector every slice shares -- an unconditional load behind the Philox block, no LDS copy: 40 KB a slice at n =
// 10^4), scale h_i as an integer, and h_eff = h_i + k (float)a_i in fp32 (one rounding).  A round then touches LDS only:
// dot_i = (F_i - scale h_i) / scale, an exact integer (subtract, shift), and field_rule_accept on (double)dot + (double)h_eff
// -- in SGA_ARITH_F32 that sum rounded to fp32 once, which is the oracle's fp32 add because dot is an integer below 2^24.
// h_eff is no integer, so there is no accept table: every uphill candidate evaluates the rule, 128 of them at once.
// On accept the tracked energy moves by the classical dE (h_i in place of h_eff), formed once for the accepted candidate.
//
// Not here: several accepts per round (sweep_clfb_impl.h) and the eight-wave tail logic of the classical sweep.
#include "sga_quantum.h"
#include "sweep_clf_impl.h"

namespace sga {

namespace {

template <typename JT, typename FT, bool F32, int CLF_BATCH, bool TAIL>
__global__ void __launch_bounds__(64 * CLF_MAX_WAVES) sweep_transverse_clf_kernel(const SweepArgs a, const TrotterLaunch q) {
    constexpr int EPL = 16 / (int)sizeof(JT), EPC = 64 * EPL;  // elements per lane / per 1-KiB chunk
    constexpr int FB = (int)sizeof(FT);
    constexpr int arith = F32 ? SGA_ARITH_F32 : SGA_ARITH_F64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const long long bits_bytes = transverse_dense_bits_bytes(a.sstride);
    FT *F = reinterpret_cast<FT *>(smem);
    unsigned int *bits = reinterpret_cast<unsigned int *>(smem + clf_bits_offset(a.ldf, FB));
    unsigned int *nup = reinterpret_cast<unsigned int *>(smem + clf_bits_offset(a.ldf, FB) + bits_bytes);
    unsigned int *ndn = reinterpret_cast<unsigned int *>(smem + clf_bits_offset(a.ldf, FB) + 2 * bits_bytes);
    int *slots2 = reinterpret_cast<int *>(smem + clf_bits_offset(a.ldf, FB) + 3 * bits_bytes);  // [2][CLF_MAX_WAVES][CLF_SLOT_INTS]

    const int tid = threadIdx.x, lane = tid & 63;
    const int W = (int)(blockDim.x >> 6);
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const MovingSlice sl = moving_slice((int)blockIdx.x, q.n_slices, q.parity);
    const int r = sl.r, n = a.n;
    const int sc = a.field_scale, sh = sc >> 1;  // scale 1 | 2: the division is a shift by 0 | 1
    const float kp = q.k_perp[sl.g];

    {   // resident state -> LDS; the neighbours' spins as bits, read-only for the launch
        const int4 *src = reinterpret_cast<const int4 *>(reinterpret_cast<const FT *>(a.fields) + (long long)r * a.ldf);
        int4 *dst = reinterpret_cast<int4 *>(F);
        for (int i = tid; i < (int)(a.ldf * FB / 16); i += blockDim.x) dst[i] = src[i];
        spins_to_bits(a.spins + (long long)r * a.sstride, bits, a.sstride, tid, blockDim.x);
        spins_to_bits(a.spins + (long long)sl.up * a.sstride, nup, a.sstride, tid, blockDim.x);
        spins_to_bits(a.spins + (long long)sl.dn * a.sstride, ndn, a.sstride, tid, blockDim.x);
    }
    __syncthreads();

    const JT *Jbase = reinterpret_cast<const JT *>(a.J);
    const int n_chunks = (int)((a.ldj + EPC - 1) / EPC);
    const double T = a.rep_temp[r];
    double E = a.energy[r];
    unsigned long long nacc = 0;

    // A row is dealt to the waves in 1-KiB chunks, chunk c -> wave c mod W, the first CLF_BATCH chunks of a wave requested
    // together into registers by unconditional loads (sweep_clf_impl.h)
    using vec_t = typename std::conditional<sizeof(JT) == 4, float4, int4>::type;
    struct RowRegs {
        vec_t x[CLF_BATCH];
    };
    auto elem0 = [&](int c) -> long long { return ((long long)c * 64 + lane) * EPL; };
    unsigned int req_off[CLF_BATCH];
#pragma unroll
    for (int b = 0; b < CLF_BATCH; ++b) {
        const long long j0 = elem0(w + b * W);
        req_off[b] = (unsigned int)((j0 < a.ldj ? j0 : 0) * (long long)sizeof(JT));
    }
    const unsigned int pitch = (unsigned int)(a.ldj * (long long)sizeof(JT));
    auto row_request = [&](int site) -> RowRegs {
        RowRegs o;
        const unsigned char *row = reinterpret_cast<const unsigned char *>(Jbase) + (unsigned long long)(unsigned int)site * pitch;
#pragma unroll
        for (int b = 0; b < CLF_BATCH; ++b) {
            unsigned int off = req_off[b];
            asm volatile("" : "+v"(off));  // (kept a 32-bit value: the scalar-base form of global_load)
            o.x[b] = *reinterpret_cast<const vec_t *>(row + off);
        }
        return o;
    };
    auto apply_chunk = [&](const vec_t &x, long long j0, int mult /* -2 scale s_i(old) */, auto neg) {
        clf_apply_chunk<JT, FT, decltype(neg)::value>(F, x, j0, mult, sc);
    };
    int nfull = 0;  // chunks of this wave's first batch that lie fully inside the row (wave-uniform)
#pragma unroll
    for (int b = 0; b < CLF_BATCH; ++b)
        if ((long long)(w + b * W + 1) * EPC <= a.ldj) nfull = b + 1;
    auto first_chunk = [&](int b) -> long long { return elem0(w + b * W); };
    auto apply_row_signed = [&](const RowRegs &rr, int site, int mult, auto neg) {
        if (!TAIL && nfull == CLF_BATCH) {
            clf_apply_full_chunks<JT, FT, decltype(neg)::value, CLF_BATCH>(F, rr.x, first_chunk, mult, sc);
        } else if (!TAIL && nfull == CLF_BATCH - 1) {
            clf_apply_full_chunks<JT, FT, decltype(neg)::value, CLF_BATCH - 1>(F, rr.x, first_chunk, mult, sc);
            const long long j0 = elem0(w + (CLF_BATCH - 1) * W);
            if (j0 < a.ldj) apply_chunk(rr.x[CLF_BATCH - 1], j0, mult, neg);
        } else {
#pragma unroll
            for (int b = 0; b < CLF_BATCH; ++b) {
                const long long j0 = elem0(w + b * W);
                if (j0 < a.ldj) apply_chunk(rr.x[b], j0, mult, neg);
            }
        }
        if constexpr (!TAIL) return;
        const JT *row = Jbase + (long long)site * a.ldj;
        for (int c0 = w + CLF_BATCH * W; c0 < n_chunks; c0 += CLF_BATCH * W) {  // (long rows only)
            vec_t x[CLF_BATCH];
#pragma unroll
            for (int b = 0; b < CLF_BATCH; ++b) {
                const long long j0 = elem0(c0 + b * W);
                x[b] = *reinterpret_cast<const vec_t *>(row + (j0 < a.ldj ? j0 : 0));
            }
#pragma unroll
            for (int b = 0; b < CLF_BATCH; ++b) {
                const long long j0 = elem0(c0 + b * W);
                if (j0 < a.ldj) apply_chunk(x[b], j0, mult, neg);
            }
        }
    };
    auto apply_row = [&](const RowRegs &rr, int site, int mult) {
        if (mult < 0) apply_row_signed(rr, site, mult, std::true_type{});  // wave-uniform
        else apply_row_signed(rr, site, mult, std::false_type{});
    };

    // what a candidate's site fixes for the whole super-window
    struct SiteConst {
        float h;      // h_i: the classical field, for the accepted candidate's dE
        float h_eff;  // h_i + k a_i in fp32
        int hq;       // scale h_i, an integer
    };
    // one candidate against the current state: the exact row sum and the spin, and whether it flips
    struct Verdict {
        int dot, si;
    };
    auto decide2 = [&](int sA, float uA, bool liveA, const SiteConst &cA, Verdict &vA, int sB, float uB, bool liveB,
                       const SiteConst &cB, Verdict &vB, bool &fA, bool &fB) {
        const int fa = (int)F[sA], fb = (int)F[sB];
        const unsigned int wa = bits[sA >> 5], wb = bits[sB >> 5];
        vA.si = ((wa >> (sA & 31)) & 1u) ? -1 : 1;
        vB.si = ((wb >> (sB & 31)) & 1u) ? -1 : 1;
        vA.dot = (fa - cA.hq) >> sh;  // (F - scale h is scale times an integer: the shift is exact)
        vB.dot = (fb - cB.hq) >> sh;
        double dA, dB;
        fA = liveA && field_rule_accept(SGA_RULE_METROPOLIS, arith, (double)vA.dot + (double)cA.h_eff, vA.si, T, uA, dA);
        fB = liveB && field_rule_accept(SGA_RULE_METROPOLIS, arith, (double)vB.dot + (double)cB.h_eff, vB.si, T, uB, dB);
    };
    // the classical dE of a flip of s_i: the rule's expression with h_i (wave-uniform arguments)
    auto classical_dE = [&](int dot, int si, float h) -> double {
        if constexpr (F32) return (double)((2.0f * (float)si) * (h + (float)dot));
        else return 2.0 * (double)si * ((double)dot + (double)h);
    };
    int turn = 0;
    constexpr int NONE = 1 << 20;

    // W consecutive windows at a time, one per wave: positions [0, 128 W) of the super-window
    for (int t0 = 0; t0 < n; t0 += CLF_WINDOW * W) {
        const int gA = w * CLF_WINDOW + 2 * lane, gB = gA + 1;  // positions in the super-window
        const int tA = t0 + gA, tB = tA + 1;
        const bool vA = tA < n, vB = tB < n;
        int sA, sB;
        float uA, uB;
        {
            // the production stream's block of updates tA, tB (the key made opaque here, as in sweep_clf_kernel: its ten
            // round values are then formed by scalar adds on the spot, not hoisted out of the loop and spilled)
            SweepArgs ak = a;
            asm volatile("" : "+s"(ak.seed_lo), "+s"(ak.seed_hi));
            const u32x4 x = sweep_block(ak, r, 0, (uint32_t)(tA >> 1));
            sA = (int)word_to_site(x.x, (uint32_t)n);  // (below n whatever the position: the loads below need no guard)
            sB = (int)word_to_site(x.z, (uint32_t)n);
            uA = word_to_u(x.y);
            uB = word_to_u(x.w);
        }
        SiteConst cA, cB;
        {
            cA.h = a.h[sA], cB.h = a.h[sB];
            const int aA = 2 - 2 * (int)(((nup[sA >> 5] >> (sA & 31)) & 1u) + ((ndn[sA >> 5] >> (sA & 31)) & 1u));
            const int aB = 2 - 2 * (int)(((nup[sB >> 5] >> (sB & 31)) & 1u) + ((ndn[sB >> 5] >> (sB & 31)) & 1u));
            cA.h_eff = cA.h + kp * (float)aA;  // the product is exact: one rounding
            cB.h_eff = cB.h + kp * (float)aB;
            cA.hq = (int)((float)sc * cA.h);   // h is a multiple of 1 / scale: exact
            cB.hq = (int)((float)sc * cB.h);
        }
        int pos = 0;  // super-window positions below pos are decided
        // one row request per round, the row of the predicted next accept travelling while the current one is applied;
        // the two row buffers take turns (sweep_clf_impl.h)
        RowRegs buf0 = row_request(0), buf1 = buf0;
        int held_pos = -1;
        auto first_of = [](unsigned long long mA, unsigned long long mB) -> int {
            const int pA = mA ? 2 * (int)__builtin_ctzll(mA) : NONE;
            const int pB = mB ? 2 * (int)__builtin_ctzll(mB) + 1 : NONE;
            return min(pA, pB);
        };
        auto round = [&](RowRegs &held, RowRegs &other) -> bool {
            int p = NONE, p2 = NONE, site = 0, site2 = 0;
            int s_old = 1;
            double dE = 0.0;
            Verdict vdA{0, 1}, vdB{0, 1};
            unsigned long long mA = 0ull, mB = 0ull;
            if ((w + 1) * CLF_WINDOW > pos) {  // wave-uniform
                bool fA, fB;
                decide2(sA, uA, vA && gA >= pos, cA, vdA, sB, uB, vB && gB >= pos, cB, vdB, fA, fB);
                mA = ballot64(fA), mB = ballot64(fB);
                p = first_of(mA, mB);
            }
            if (p < NONE) {
                if (p & 1) mB &= mB - 1;
                else mA &= mA - 1;
                p2 = first_of(mA, mB);
                site = __builtin_amdgcn_readlane((p & 1) ? sB : sA, p >> 1);
                s_old = __builtin_amdgcn_readlane((p & 1) ? vdB.si : vdA.si, p >> 1);
                dE = classical_dE(__builtin_amdgcn_readlane((p & 1) ? vdB.dot : vdA.dot, p >> 1), s_old,
                                  read_lane((p & 1) ? cB.h : cA.h, p >> 1));
                if (p2 < NONE) site2 = __builtin_amdgcn_readlane((p2 & 1) ? sB : sA, p2 >> 1);
                p += w * CLF_WINDOW;
                if (p2 < NONE) p2 += w * CLF_WINDOW;
            }
            if (W > 1) {
                int *slots = slots2 + turn * (CLF_SLOT_INTS * CLF_MAX_WAVES);
                turn ^= 1;
                if (lane == 0) {
                    int4 *mine = reinterpret_cast<int4 *>(slots + CLF_SLOT_INTS * w);
                    const long long dbits = __double_as_longlong(dE);
                    mine[0] = make_int4(p, p2, site, site2);
                    mine[1] = make_int4((int)(unsigned int)dbits, (int)(dbits >> 32), s_old, 0);
                }
                __syncthreads();  // (A) every wave has evaluated against the old state and published
                int4 q0 = make_int4(NONE, NONE, 0, 0), q1 = make_int4(0, 0, 1, 0);
                if (lane < W) {
                    const int4 *theirs = reinterpret_cast<const int4 *>(slots + CLF_SLOT_INTS * lane);
                    q0 = theirs[0], q1 = theirs[1];
                }
                const unsigned long long have = ballot64(q0.x < NONE);
                if (have == 0ull) {
                    p = NONE;
                } else {
                    const int win = (int)__builtin_ctzll(have);
                    p = __builtin_amdgcn_readlane(q0.x, win), p2 = __builtin_amdgcn_readlane(q0.y, win);
                    site = __builtin_amdgcn_readlane(q0.z, win), site2 = __builtin_amdgcn_readlane(q0.w, win);
                    const unsigned int dlo = (unsigned int)__builtin_amdgcn_readlane(q1.x, win);
                    const unsigned int dhi = (unsigned int)__builtin_amdgcn_readlane(q1.y, win);
                    dE = __longlong_as_double((long long)(((unsigned long long)dhi << 32) | dlo));
                    s_old = __builtin_amdgcn_readlane(q1.z, win);
                    const unsigned long long later = have & (have - 1);
                    if (p2 >= NONE && later) {
                        const int nx = (int)__builtin_ctzll(later);
                        p2 = __builtin_amdgcn_readlane(q0.x, nx), site2 = __builtin_amdgcn_readlane(q0.z, nx);
                    }
                }
            }
            if (p >= NONE) return true;  // the rest of the super-window is rejected
            if (held_pos != p) held = row_request(site);
            other = row_request(p2 < NONE ? site2 : site);
            held_pos = p2 < NONE ? p2 : -1;
            E += dE;
            ++nacc;
            apply_row(held, site, -2 * sc * s_old);
            if (tid == 0) bits[site >> 5] ^= 1u << (site & 31);
            pos = p + 1;
            __syncthreads();  // (B) fields and spin of the new state are visible
            return pos >= CLF_WINDOW * W;
        };
        for (;;) {
            if (round(buf0, buf1)) break;
            if (round(buf1, buf0)) break;
        }
    }

    // the slice moved in this half-sweep only: its energy now is its energy at the sweep's end, where the best follows
    double bestE = a.best_energy[r];
    if (E < bestE) {
        bestE = E;
        bits_to_spins(bits, a.best_spins + (long long)r * a.sstride, a.sstride, n, tid, blockDim.x);
    }
    __syncthreads();
    {
        int4 *dst = reinterpret_cast<int4 *>(reinterpret_cast<FT *>(a.fields) + (long long)r * a.ldf);
        const int4 *src = reinterpret_cast<const int4 *>(F);
        for (int i = tid; i < (int)(a.ldf * FB / 16); i += blockDim.x) dst[i] = src[i];
        bits_to_spins(bits, a.spins + (long long)r * a.sstride, a.sstride, n, tid, blockDim.x);
    }
    if (tid == 0) {
        a.energy[r] = E;
        a.best_energy[r] = bestE;
        a.n_accepted[r] += nacc;
    }
}

template <typename JT, typename FT, bool F32>
hipError_t launch_tclf(const SweepArgs &a, const TrotterLaunch &t, int waves, hipStream_t st) {
    const size_t lds = transverse_dense_lds_bytes(a.ldf, (int)sizeof(FT), a.sstride);
    if (lds > TRANSVERSE_LDS_BUDGET) return hipErrorInvalidValue;
    const int batch = sweep_clf_batch(a.ldj, sizeof(JT) == 1, waves);
    const int epc = sizeof(JT) == 1 ? 1024 : 256;
    const bool tail = (int)((a.ldj + epc - 1) / epc) > batch * waves;  // (never with 3 chunks per wave)
    void (*kern)(const SweepArgs, const TrotterLaunch) =
        batch == 3 ? sweep_transverse_clf_kernel<JT, FT, F32, 3, false>
        : tail     ? sweep_transverse_clf_kernel<JT, FT, F32, CLF_BATCH_MAX, true>
                   : sweep_transverse_clf_kernel<JT, FT, F32, CLF_BATCH_MAX, false>;
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(t.moving), dim3(64 * waves), lds, st, a, t);
    note_sweep_kernel("sweep_transverse_clf_kernel<%s, %s, %s, BATCH=%d, TAIL=%d, %d slices, parity %d> x %d wave(s)",
                      sizeof(JT) == 4 ? "float" : "int8_t", sizeof(FT) == 2 ? "int16_t" : "int32_t", F32 ? "f32 rule" : "f64 rule",
                      batch, (int)tail, t.n_slices, t.parity, waves);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sweep_transverse_dense(const SweepArgs &a, const TrotterLaunch &t, bool j_is_i8, int waves, hipStream_t st) {
    if (waves < 1 || waves > CLF_MAX_WAVES || !a.J || !a.h || !a.spins || !a.best_spins || !a.fields || !t.k_perp ||
        (a.field_bits != 16 && a.field_bits != 32) || (a.field_scale != 1 && a.field_scale != 2) ||
        (a.ldf * (a.field_bits / 8)) % 16 != 0 || a.sstride % 32 != 0 || a.sstride < a.n || a.ldf < a.ldj || a.ldj < a.n ||
        (a.ldj * (j_is_i8 ? 1 : 4)) % 16 != 0 || a.n < 1 || t.n_slices < 2 || (t.n_slices & 1) || a.R % t.n_slices != 0 ||
        t.moving != a.R / 2 || (t.parity != 0 && t.parity != 1))
        return hipErrorInvalidValue;
    const bool f32 = a.arith == SGA_ARITH_F32;
    // (built per arithmetic, as sweep_transverse_kernel is: with a run-time arith both rules' code stays live in the round)
    if (j_is_i8) {
        if (a.field_bits == 16) return f32 ? launch_tclf<int8_t, int16_t, true>(a, t, waves, st) : launch_tclf<int8_t, int16_t, false>(a, t, waves, st);
        return f32 ? launch_tclf<int8_t, int32_t, true>(a, t, waves, st) : launch_tclf<int8_t, int32_t, false>(a, t, waves, st);
    }
    if (a.field_bits == 16) return f32 ? launch_tclf<float, int16_t, true>(a, t, waves, st) : launch_tclf<float, int16_t, false>(a, t, waves, st);
    return f32 ? launch_tclf<float, int32_t, true>(a, t, waves, st) : launch_tclf<float, int32_t, false>(a, t, waves, st);
}

}  // namespace sga
