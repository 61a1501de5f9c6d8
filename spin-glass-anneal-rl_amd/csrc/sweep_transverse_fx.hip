// sweep_transverse_fx.hip -- simulated quantum annealing on DENSE couplings with REAL-VALUED J, carried by the fixed-point
// cached fields (sga_sweep_transverse_dense under option "clf_fixed_point").
//
// The step is sweep_transverse_clf.hip's, word for word: groups of P slices, one launch is one HALF-SWEEP, the slices of
// one parity move through the n updates of the production stream while their neighbours stand still, a_i = s_up[i] +
// s_dn[i] is a constant of the launch and h_eff = h_i + k (float)a_i one fp32 rounding.  The fields are sweep_clf_fx.hip's:
// D = 2^k J s kept EXACTLY as int32 | int64 in LDS (a.field_scale = k), h never folded in -- so h may be any fp32 and J
// any matrix of the exact accumulation classes (quarter-valued penalties, binary-grid couplings, integer J beside a
// real-valued h).  A candidate's decision is the classical fixed-point kernel's call with h_eff in place of h_i:
//     dot = fp32(2^-k D_i)  (the row kernels' dotf: one rounding of the exact row sum),
//     metropolis_accept(SGA_RULE_METROPOLIS, arith, dot, s_i, h_eff, 0, T, u, .)
// and on accept the tracked energy moves by the classical dE -- the rule's dE expression with h_i, formed once for the
// winning candidate -- E += dE in chain order.  The neighbour term stays outside D: a rejected proposal leaves the state
// untouched and the window logic carries over as it stands.
//
// From the transverse kernel: one workgroup per moving slice, the two neighbour slices' spins staged once per launch as
// bits, h gathered once per super-window behind the Philox block, (h_i, h_eff) in registers, the slot exchange and its
// two barriers, the predicted next accept's row requested one round ahead, the opaque Philox key.  From the fixed-point
// kernel: dot_of (int -> fp64 -> ldexp -> fp32) and fx_apply_chunk (wrapping unsigned adds of -2 s_i 2^k J_ij, each entry
// scaled exactly by fp64 ldexp), int8 rows for integer J.
//
// Builds: (int8 rows, int32 fields), (fp32 rows, int32 fields), (fp32 rows, int64 fields).  int8 rows with int64 fields
// cannot occur: |J| <= 127 and n <= 37 000 (the LDS bound) keep 2^0 sum_j |J_ij| below 2^31.
#include "sga_quantum.h"
#include "sweep_clf_fx_impl.h"

namespace sga {

namespace {

template <typename JT, typename FT, bool F32, int BATCH, bool TAIL>
__global__ void __launch_bounds__(64 * CLF_MAX_WAVES) sweep_transverse_fx_kernel(const SweepArgs a, const TrotterLaunch q) {
    constexpr int EPL = 16 / (int)sizeof(JT), EPC = 64 * EPL;  // elements per lane / per 1-KiB chunk
    constexpr int FB = (int)sizeof(FT);
    constexpr int arith = F32 ? SGA_ARITH_F32 : SGA_ARITH_F64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const long long bits_bytes = transverse_dense_bits_bytes(a.sstride);
    FT *F = reinterpret_cast<FT *>(smem);  // D = 2^kx J s of the moving slice
    unsigned int *bits = reinterpret_cast<unsigned int *>(smem + clf_bits_offset(a.ldf, FB));
    unsigned int *nup = reinterpret_cast<unsigned int *>(smem + clf_bits_offset(a.ldf, FB) + bits_bytes);
    unsigned int *ndn = reinterpret_cast<unsigned int *>(smem + clf_bits_offset(a.ldf, FB) + 2 * bits_bytes);
    int *slots2 = reinterpret_cast<int *>(smem + clf_bits_offset(a.ldf, FB) + 3 * bits_bytes);  // [2][CLF_MAX_WAVES][CLF_SLOT_INTS]

    const int tid = threadIdx.x, lane = tid & 63;
    const int W = (int)(blockDim.x >> 6);
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const MovingSlice sl = moving_slice((int)blockIdx.x, q.n_slices, q.parity);
    const int r = sl.r, n = a.n;
    const int kx = a.field_scale;
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

    // A row is dealt to the waves in 1-KiB chunks, chunk c -> wave c mod W, the first BATCH chunks of a wave requested
    // together into registers by unconditional loads (a lane past the row's end reads the row's first granule)
    using vec_t = typename std::conditional<sizeof(JT) == 4, float4, int4>::type;
    struct RowRegs {
        vec_t x[BATCH];
    };
    auto elem0 = [&](int c) -> long long { return ((long long)c * 64 + lane) * EPL; };
    unsigned int req_off[BATCH];
#pragma unroll
    for (int b = 0; b < BATCH; ++b) {
        const long long j0 = elem0(w + b * W);
        req_off[b] = (unsigned int)((j0 < a.ldj ? j0 : 0) * (long long)sizeof(JT));
    }
    const unsigned int pitch = (unsigned int)(a.ldj * (long long)sizeof(JT));
    auto row_request = [&](int site) -> RowRegs {
        RowRegs o;
        const unsigned char *row = reinterpret_cast<const unsigned char *>(Jbase) + (unsigned long long)(unsigned int)site * pitch;
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
            unsigned int off = req_off[b];
            asm volatile("" : "+v"(off));  // (kept a 32-bit value: the scalar-base form of global_load)
            o.x[b] = *reinterpret_cast<const vec_t *>(row + off);
        }
        return o;
    };
    auto apply_row = [&](const RowRegs &rr, int site, int mult /* -2 s_i(old) */) {
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
            const long long j0 = elem0(w + b * W);
            if (j0 < a.ldj) fx_apply_chunk<JT, FT>(F, rr.x[b], j0, mult, kx);
        }
        if constexpr (!TAIL) return;
        const JT *row = Jbase + (long long)site * a.ldj;
        for (int c0 = w + BATCH * W; c0 < n_chunks; c0 += BATCH * W) {  // (long rows only)
            vec_t x[BATCH];
#pragma unroll
            for (int b = 0; b < BATCH; ++b) {
                const long long j0 = elem0(c0 + b * W);
                x[b] = *reinterpret_cast<const vec_t *>(row + (j0 < a.ldj ? j0 : 0));
            }
#pragma unroll
            for (int b = 0; b < BATCH; ++b) {
                const long long j0 = elem0(c0 + b * W);
                if (j0 < a.ldj) fx_apply_chunk<JT, FT>(F, x[b], j0, mult, kx);
            }
        }
    };

    // what a candidate's site fixes for the whole super-window
    struct SiteConst {
        float h;      // h_i: the classical field, for the accepted candidate's dE
        float h_eff;  // h_i + k a_i in fp32
    };
    // one candidate against the current state: the row kernels' dot and the spin
    struct Verdict {
        float dot;
        int si;
    };
    // the row kernels' dot: the exact sum rounded to fp32 once
    auto dot_of = [&](int s) -> float { return (float)ldexp((double)F[s], -kx); };
    auto spin_of = [&](int s) -> int { return ((bits[s >> 5] >> (s & 31)) & 1u) ? -1 : 1; };
    // the classical dE of a flip of s_i: the rule's expression with h_i and a zero diagonal (wave-uniform arguments)
    auto classical_dE = [&](float dot, int si, float h) -> double {
        if constexpr (F32) return (double)((2.0f * (float)si) * (h + dot));
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
            // the production stream's block of updates tA, tB (the key made opaque, as in sweep_transverse_clf_kernel)
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
            if ((w + 1) * CLF_WINDOW > pos) {  // wave-uniform
                Verdict vdA, vdB;
                vdA.si = spin_of(sA), vdB.si = spin_of(sB);
                vdA.dot = dot_of(sA), vdB.dot = dot_of(sB);
                double dA, dB;  // (the rule's dE under h_eff: not the tracked energy's)
                const bool fA = (vA && gA >= pos) && metropolis_accept(SGA_RULE_METROPOLIS, arith, vdA.dot, vdA.si, cA.h_eff, 0.0f, T, uA, dA);
                const bool fB = (vB && gB >= pos) && metropolis_accept(SGA_RULE_METROPOLIS, arith, vdB.dot, vdB.si, cB.h_eff, 0.0f, T, uB, dB);
                unsigned long long mA = ballot64(fA), mB = ballot64(fB);
                p = first_of(mA, mB);
                if (p < NONE) {
                    if (p & 1) mB &= mB - 1;
                    else mA &= mA - 1;
                    p2 = first_of(mA, mB);
                    site = __builtin_amdgcn_readlane((p & 1) ? sB : sA, p >> 1);
                    s_old = __builtin_amdgcn_readlane((p & 1) ? vdB.si : vdA.si, p >> 1);
                    dE = classical_dE(read_lane((p & 1) ? vdB.dot : vdA.dot, p >> 1), s_old, read_lane((p & 1) ? cB.h : cA.h, p >> 1));
                    if (p2 < NONE) site2 = __builtin_amdgcn_readlane((p2 & 1) ? sB : sA, p2 >> 1);
                    p += w * CLF_WINDOW;
                    if (p2 < NONE) p2 += w * CLF_WINDOW;
                }
            }
            if (W > 1) {  // the earliest window with an accept decides (sweep_clf_impl.h)
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
            E += dE;  // (in chain order, as the row kernels add it)
            ++nacc;
            apply_row(held, site, -2 * s_old);
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
hipError_t launch_tfx(const SweepArgs &a, const TrotterLaunch &t, int waves, hipStream_t st) {
    const size_t lds = transverse_dense_lds_bytes(a.ldf, (int)sizeof(FT), a.sstride);
    if (lds > TRANSVERSE_LDS_BUDGET) return hipErrorInvalidValue;
    // (int8 rows: three chunks per request, as sweep_clf_fx_kernel has them -- five hold 2 x 80 bytes of row per lane)
    const int batch = sizeof(JT) == 1 ? 3 : sweep_clf_batch(a.ldj, false, waves);
    const int epc = sizeof(JT) == 1 ? 1024 : 256;
    const bool tail = (int)((a.ldj + epc - 1) / epc) > batch * waves;
    void (*kern)(const SweepArgs, const TrotterLaunch) = nullptr;
    if constexpr (sizeof(JT) == 1) {
        kern = tail ? sweep_transverse_fx_kernel<JT, FT, F32, 3, true> : sweep_transverse_fx_kernel<JT, FT, F32, 3, false>;
    } else {  // (fp32 rows: never a tail with 3 chunks per wave)
        kern = batch == 3 ? sweep_transverse_fx_kernel<JT, FT, F32, 3, false>
               : tail     ? sweep_transverse_fx_kernel<JT, FT, F32, CLF_BATCH_MAX, true>
                          : sweep_transverse_fx_kernel<JT, FT, F32, CLF_BATCH_MAX, false>;
    }
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(t.moving), dim3(64 * waves), lds, st, a, t);
    note_sweep_kernel("sweep_transverse_fx_kernel<%s, %s, %s, BATCH=%d, TAIL=%d, k=%d, %d slices, parity %d> x %d wave(s)",
                      sizeof(JT) == 4 ? "float" : "int8_t", sizeof(FT) == 4 ? "int32_t" : "int64_t", F32 ? "f32 rule" : "f64 rule",
                      batch, (int)tail, a.field_scale, t.n_slices, t.parity, waves);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sweep_transverse_dense_fx(const SweepArgs &a, const TrotterLaunch &t, bool j_is_i8, int waves, hipStream_t st) {
    if (waves < 1 || waves > CLF_MAX_WAVES || !a.J || !a.h || !a.spins || !a.best_spins || !a.fields || !t.k_perp ||
        (a.field_bits != 32 && a.field_bits != 64) || a.field_scale < 0 || (j_is_i8 && (a.field_scale != 0 || a.field_bits != 32)) ||
        (a.ldf * (a.field_bits / 8)) % 16 != 0 || a.sstride % 32 != 0 || a.sstride < a.n || a.ldf < a.ldj || a.ldj < a.n ||
        (a.ldj * (j_is_i8 ? 1 : 4)) % 16 != 0 || a.n < 1 || t.n_slices < 2 || (t.n_slices & 1) || a.R % t.n_slices != 0 ||
        t.moving != a.R / 2 || (t.parity != 0 && t.parity != 1))
        return hipErrorInvalidValue;
    const bool f32 = a.arith == SGA_ARITH_F32;
    // (built per arithmetic, as the sibling is: with a run-time arith both rules' code stays live in the round)
    if (j_is_i8) return f32 ? launch_tfx<int8_t, int, true>(a, t, waves, st) : launch_tfx<int8_t, int, false>(a, t, waves, st);
    if (a.field_bits == 32) return f32 ? launch_tfx<float, int, true>(a, t, waves, st) : launch_tfx<float, int, false>(a, t, waves, st);
    return f32 ? launch_tfx<float, long long, true>(a, t, waves, st) : launch_tfx<float, long long, false>(a, t, waves, st);
}

}  // namespace sga
