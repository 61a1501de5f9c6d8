// sweep_groups.hip -- single-spin sweeps on couplings that are a sum of complete graphs on groups of sites and are
// never stored (sga_set_groups: the assignment and scheduling instances, BASELINE configs[1] / configs[3], whose every
// coupling comes from a cardinality constraint):
//     J_ij = sum_{g contains i and j} c_g   (i != j),   J_ii = 0
//     sum_j J_ij s_j = sum_{g contains i} c_g (S_g - s_i),   S_g = sum_{j in g} s_j.
// Per replica the kernel keeps the spins as bits and the group sums S_g as integers (int16 | int32) in LDS.  A
// proposal at site i reads the K_i sums of its groups; an accept flips one bit and moves K_i integers.  No coupling
// byte is read from HBM: the site -> group table (gptr[n + 1], entries (group, coefficient) interleaved) is all a
// sweep fetches, through the caches.
//
// Arithmetic: the engine checks at set time that every c_g is an integer multiple of one 2^-k and that
// 2^k max_i sum_{g contains i} |c_g| (|g| - 1) < 2^24.  Then every product c_g (S_g - s_i) and every partial sum of a
// row is an integer multiple of 2^-k below 2^24 2^-k: exact in fp32 in ANY order.  The stored forms' fp32 row sum of
// the materialised couplings is exact under the same bound, so the two are the same number and the chains agree bit
// for bit.
//
// Production form (Philox sites, Metropolis, no traces): W waves per replica.  Wave w of a super-window holds the
// 128 updates of Philox blocks 64 (W m + w) ... + 63 (lane l: updates 2 l and 2 l + 1 of the window), evaluates all of
// them against the sums as they stand, a ballot finds the wave's first accept, the waves meet in LDS decision slots,
// the first accept of the super-window is applied (one bit, K_i sums), and only the candidates behind it are
// evaluated again.  A super-window costs (accepts + 1) rounds whatever the number of proposals.
// General form: one wave, one update at a time: sequential / replayed sites, Glauber / heat bath, fp32 operator
// arithmetic, per-update traces.
//
// Stored remainder (sga_set_groups_csr, template flag REST): J_ij = sum_g c_g + R_ij with R a CSR matrix in HBM
// (rptr[n + 1], (column, value bits) entries, rows strictly sorted, symmetric, zero diagonal, at most
// GROUPS_MAX_REST_ROW entries per row).  The set-time bound covers both parts -- every c_g and R_ij a multiple of one
// 2^-k, 2^k max_i (sum_g |c_g| (|g| - 1) + sum_j |R_ij|) < 2^24 -- so the combined row sum is exact in any order too.
// The general, energy and field kernels add a walk of the site's remainder row against the spin bits.  The production
// form walks a candidate's row ONCE per super-window (rd = sum_j R_ij s_j, in request()); an accept at site a is
// published with its old spin, and every still-undecided candidate looks a up in its own sorted row (<= 8 probes)
// and moves rd by -2 R_ia s_a: rounds stay (accepts + 1), not (accepts + 1) x row length.
#include "sweep_common.h"

namespace sga {

constexpr int GROUPS_MAX_WAVES = 8;
constexpr int GROUPS_REG_ENTRIES = 4;  // memberships of a candidate held in registers (the rest re-read through L1)

template <bool WIDE>
struct GroupSums {
    using type = typename std::conditional<WIDE, int, short>::type;
};

// bits | sums | decision slots [2][GROUPS_MAX_WAVES] ints | accepted update (dE: 2 ints, 2 pad) [2]
size_t groups_lds_bytes(int sstride, int n_groups, int wide) {
    const size_t sums = ((size_t)n_groups * (wide ? 4 : 2) + 15) & ~(size_t)15;
    return (size_t)sstride / 8 + sums + 2 * GROUPS_MAX_WAVES * sizeof(int) + 2 * 4 * sizeof(int);
}

// S_g of the replica from its spin bits: one thread per group, members in storage order
template <typename sum_t>
__device__ inline void groups_load_sums(const GroupArgs &g, const unsigned int *bits, sum_t *sums, int first, int step) {
    for (int q = first; q < g.n_groups; q += step) {
        int s = 0;
        for (long long m = g.member_ptr[q]; m < g.member_ptr[q + 1]; ++m) {
            const int j = g.members[m];
            s += ((bits[j >> 5] >> (j & 31)) & 1u) ? -1 : 1;
        }
        sums[q] = (sum_t)s;
    }
}

template <typename sum_t>
__device__ __forceinline__ float groups_row_sum(const GroupArgs &g, const unsigned int *bits, const sum_t *sums, int site,
                                                int &si) {
    si = ((bits[site >> 5] >> (site & 31)) & 1u) ? -1 : 1;
    float acc = 0.0f;
    for (int m = g.gptr[site]; m < g.gptr[site + 1]; ++m) {
        const int2 ent = g.gent[m];
        acc += __int_as_float(ent.y) * (float)((int)sums[ent.x] - si);  // exact (set-time bound)
    }
    return acc;
}

// the flip of `site` (one lane): its bit, and S_g -= 2 s_i for every group of the site
template <typename sum_t>
__device__ __forceinline__ void groups_apply(const GroupArgs &g, unsigned int *bits, sum_t *sums, int site, int si) {
    atomicXor(&bits[site >> 5], 1u << (site & 31));
    for (int m = g.gptr[site]; m < g.gptr[site + 1]; ++m) {
        const int q = g.gent[m].x;
        sums[q] = (sum_t)((int)sums[q] - 2 * si);
    }
}

// sum_j R_ij s_j of one site (one lane walks the row; exact under the set-time bound)
__device__ __forceinline__ float groups_rest_row_sum(const GroupArgs &g, const unsigned int *bits, int site) {
    float acc = 0.0f;
    for (int m = g.rest.rptr[site]; m < g.rest.rptr[site + 1]; ++m) {
        const int2 ent = g.rest.rent[m];
        acc += ((bits[ent.x >> 5] >> (ent.x & 31)) & 1u) ? -__int_as_float(ent.y) : __int_as_float(ent.y);
    }
    return acc;
}

// R_ia of a strictly sorted remainder row [beg, beg + cnt): 0 when the row has no column a
__device__ __forceinline__ float groups_rest_find(const GroupArgs &g, int beg, int cnt, int a) {
    int lo = 0, hi = cnt;  // first entry with column >= a
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (g.rest.rent[beg + mid].x < a) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= cnt) return 0.0f;
    const int2 ent = g.rest.rent[beg + lo];
    return ent.x == a ? __int_as_float(ent.y) : 0.0f;
}

// ---------------------------------------------------------------------------------------
// Production form
// ---------------------------------------------------------------------------------------
template <bool WIDE, bool REST>
__global__ void __launch_bounds__(64 * GROUPS_MAX_WAVES) sweep_groups_kernel(const SweepArgs a, const GroupArgs g) {
    using sum_t = typename GroupSums<WIDE>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned int *bits = reinterpret_cast<unsigned int *>(smem);
    sum_t *sums = reinterpret_cast<sum_t *>(smem + a.sstride / 8);
    int *dec = reinterpret_cast<int *>(smem + a.sstride / 8 + (((size_t)g.n_groups * sizeof(sum_t) + 15) & ~(size_t)15));
    int *won = dec + 2 * GROUPS_MAX_WAVES;  // [2][4]: dE of the applied update (REST: its site and old spin behind)
    const int tid = threadIdx.x, lane = tid & 63;
    const int W = (int)(blockDim.x >> 6);
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = blockIdx.x;
    spins_to_bits(a.spins + (long long)r * a.sstride, bits, a.sstride, tid, (int)blockDim.x);
    __syncthreads();
    groups_load_sums(g, bits, sums, tid, (int)blockDim.x);
    __syncthreads();

    double E = a.energy[r], bestE = a.best_energy[r], T = 1.0;
    unsigned long long nacc = 0;
    const int N = a.n;
    const int nwin = ((N + 1) / 2 + 63) / 64;      // windows of 64 Philox blocks = 128 updates per sweep
    const int nsuper = (nwin + W - 1) / W;
    constexpr int KR = GROUPS_REG_ENTRIES;
    constexpr int NONE = 1 << 20;
    int turn = 0;

    struct Cand {
        int site, beg, cnt, live;
        float u, h;
        int2 ent[KR];
        int rbeg, rcnt;  // REST: the site's remainder row ...
        float rd;        // ... and sum_j R_ij s_j against the state as it stands (moved by every accept)
    };
    auto request = [&](Cand &c) {  // what the candidate's decisions need, fetched once per window
        c.beg = g.gptr[c.site];
        c.cnt = g.gptr[c.site + 1] - c.beg;
        c.h = a.h[c.site];
#pragma unroll
        for (int q = 0; q < KR; ++q)  // past the site's memberships: group 0 with coefficient 0 adds an exact zero
            c.ent[q] = q < c.cnt ? g.gent[c.beg + q] : make_int2(0, 0);
        if constexpr (REST) {  // the applies of the previous super-window are behind barrier (B)
            c.rbeg = g.rest.rptr[c.site];
            c.rcnt = g.rest.rptr[c.site + 1] - c.rbeg;
            c.rd = c.live ? groups_rest_row_sum(g, bits, c.site) : 0.0f;
        }
    };
    auto decide = [&](const Cand &c, int &si, double &dE) -> bool {
        si = ((bits[c.site >> 5] >> (c.site & 31)) & 1u) ? -1 : 1;
        float acc = 0.0f;
#pragma unroll
        for (int q = 0; q < KR; ++q) acc += __int_as_float(c.ent[q].y) * (float)((int)sums[c.ent[q].x] - si);
        for (int q = KR; q < c.cnt; ++q) {
            const int2 ent = g.gent[c.beg + q];
            acc += __int_as_float(ent.y) * (float)((int)sums[ent.x] - si);
        }
        if constexpr (REST) acc += c.rd;
        return metropolis_accept(SGA_RULE_METROPOLIS, SGA_ARITH_F64, acc, si, c.h, 0.0f, T, c.u, dE);
    };

    for (int k = 0; k < a.n_sweeps; ++k) {
        T = a.sched ? a.sched[k * a.sched_ss + r * a.sched_rs] : a.rep_temp[r];
        for (int sw = 0; sw < nsuper; ++sw) {
            const int b = 64 * (sw * W + w) + lane;  // this lane's Philox block: updates 2 b and 2 b + 1 of the sweep
            const u32x4 x = sweep_block(a, r, k, (uint32_t)b);
            Cand c0, c1;
            c0.live = 2 * b < N;
            c1.live = 2 * b + 1 < N;
            c0.site = c0.live ? (int)word_to_site(x.x, (uint32_t)N) : 0;
            c1.site = c1.live ? (int)word_to_site(x.z, (uint32_t)N) : 0;
            c0.u = word_to_u(x.y);
            c1.u = word_to_u(x.w);
            request(c0);
            request(c1);
            int start = 0;  // candidates 2 lane + j >= start of this wave are undecided
            for (;;) {
                int s0 = 1, s1 = 1;
                double d0 = 0.0, d1 = 0.0;
                const bool f0 = c0.live && 2 * lane >= start && decide(c0, s0, d0);
                const bool f1 = c1.live && 2 * lane + 1 >= start && decide(c1, s1, d1);
                const unsigned long long b0 = ballot64(f0), b1 = ballot64(f1);
                const int i0 = b0 ? 2 * (int)__builtin_ctzll(b0) : NONE, i1 = b1 ? 2 * (int)__builtin_ctzll(b1) + 1 : NONE;
                const int mine = min(i0, i1);  // this wave's first accept against the state as it stands
                int *slot = dec + turn * GROUPS_MAX_WAVES;
                if (lane == 0) slot[w] = mine;
                __syncthreads();  // (A) every wave has decided against the same state
                int first_w = -1, first_i = NONE;
                for (int q = W - 1; q >= 0; --q) {
                    const int v = slot[q];
                    if (v != NONE) {
                        first_w = q;
                        first_i = v;
                    }
                }
                int *rec = won + turn * 4;
                turn ^= 1;
                if (first_w < 0) break;  // nothing (more) accepts in this super-window
                if (w == first_w && lane == (first_i >> 1)) {  // the owner applies its update and publishes dE
                    const bool second = first_i & 1;
                    const int site = second ? c1.site : c0.site, si = second ? s1 : s0;
                    atomicXor(&bits[site >> 5], 1u << (site & 31));
                    const Cand &c = second ? c1 : c0;
                    for (int q = 0; q < c.cnt; ++q) {
                        const int gq = g.gent[c.beg + q].x;
                        sums[gq] = (sum_t)((int)sums[gq] - 2 * si);
                    }
                    const long long db = __double_as_longlong(second ? d1 : d0);
                    rec[0] = (int)(unsigned int)db;
                    rec[1] = (int)(db >> 32);
                    if constexpr (REST) {
                        rec[2] = site;
                        rec[3] = si;
                    }
                }
                __syncthreads();  // (B) the new state and the record are visible
                E += __longlong_as_double((long long)(((unsigned long long)(unsigned int)rec[1] << 32) | (unsigned int)rec[0]));
                ++nacc;
                // waves before the accepting one are done, it goes on behind the accept, later ones start over
                start = w < first_w ? 128 : (w == first_w ? first_i + 1 : 0);
                if constexpr (REST) {  // the undecided candidates' remainder sums follow the flip of site a (diagonal 0)
                    const int sa = rec[2];
                    const float two_s = (float)(2 * rec[3]);
                    if (c0.live && 2 * lane >= start && c0.rcnt > 0) c0.rd -= two_s * groups_rest_find(g, c0.rbeg, c0.rcnt, sa);
                    if (c1.live && 2 * lane + 1 >= start && c1.rcnt > 0) c1.rd -= two_s * groups_rest_find(g, c1.rbeg, c1.rcnt, sa);
                }
            }
        }
        if (tid == 0 && a.energy_trace) a.energy_trace[(long long)k * a.R + r] = E;
        if (E < bestE && !a.no_best) {  // annealing/gpu_annealer.py:151-153
            bestE = E;
            bits_to_spins(bits, a.best_spins + (long long)r * a.sstride, a.sstride, N, tid, (int)blockDim.x);
            __syncthreads();
        }
    }
    __syncthreads();
    bits_to_spins(bits, a.spins + (long long)r * a.sstride, a.sstride, N, tid, (int)blockDim.x);
    if (tid == 0) {
        a.energy[r] = E;
        a.best_energy[r] = bestE;
        a.n_accepted[r] += nacc;
    }
}

// ---------------------------------------------------------------------------------------
// General form: one wave per replica, one update at a time; every lane walks the same chain
// ---------------------------------------------------------------------------------------
template <bool WIDE, bool REST>
__global__ void __launch_bounds__(64) sweep_groups_general_kernel(const SweepArgs a, const GroupArgs g) {
    using sum_t = typename GroupSums<WIDE>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned int *bits = reinterpret_cast<unsigned int *>(smem);
    sum_t *sums = reinterpret_cast<sum_t *>(smem + a.sstride / 8);
    const int tid = threadIdx.x;
    const int r = a.rep_list ? a.rep_list[blockIdx.x] : (int)blockIdx.x;
    const int rule = a.rule, arith = a.arith;
    spins_to_bits(a.spins + (long long)r * a.sstride, bits, a.sstride, tid, 64);
    __syncthreads();
    groups_load_sums(g, bits, sums, tid, 64);
    __syncthreads();

    double E = a.energy[r], bestE = a.best_energy[r];
    unsigned long long nacc = 0;
    const int N = a.n;
    for (int k = 0; k < a.n_sweeps; ++k) {
        const double T = a.sched ? a.sched[k * a.sched_ss + r * a.sched_rs] : a.rep_temp[r];
        UpdatePair pr{0, 0, 2.0f, 2.0f};
        for (int t = 0; t < N; ++t) {
            if (!(t & 1)) pr = fetch_pair<false>(a, r, k, t >> 1, true);
            const int site = (t & 1) ? pr.sB : pr.sA;
            const float u = (t & 1) ? pr.uB : pr.uA;
            int si;
            float dot = groups_row_sum(g, bits, sums, site, si);
            if constexpr (REST) dot += groups_rest_row_sum(g, bits, site);
            double dE;
            const bool flip = metropolis_accept(rule, arith, dot, si, a.h[site], 0.0f, T, u, dE);
            __syncthreads();  // every lane has read the old state
            if (flip) {
                E += dE;
                ++nacc;
                if (tid == 0) groups_apply(g, bits, sums, site, si);
            }
            __syncthreads();
            if (tid == 0) {
                const long long upd = (long long)r * a.replay_stride + (long long)k * N + t;
                if (a.accept_trace) a.accept_trace[upd] = flip ? 1 : 0;
                if (a.dE_trace) a.dE_trace[upd] = flip ? (rule == SGA_RULE_HEAT_BATH ? -dE : dE) : 0.0;
            }
        }
        if (tid == 0 && a.energy_trace) a.energy_trace[(long long)k * a.R + r] = E;
        if (E < bestE && !a.no_best) {
            bestE = E;
            bits_to_spins(bits, a.best_spins + (long long)r * a.sstride, a.sstride, N, tid, 64);
            __syncthreads();
        }
    }
    __syncthreads();
    bits_to_spins(bits, a.spins + (long long)r * a.sstride, a.sstride, N, tid, 64);
    if (tid == 0) {
        a.energy[r] = E;
        a.best_energy[r] = bestE;
        a.n_accepted[r] += nacc;
    }
}

hipError_t launch_sweep_groups(const SweepArgs &a, const GroupArgs &g, int waves, hipStream_t st) {
    const bool rest = g.rest.nnz > 0;
    if (waves < 1 || waves > GROUPS_MAX_WAVES || a.sstride % 128 != 0 || (g.n_groups < 1 && !rest)) return hipErrorInvalidValue;
    const size_t lds = groups_lds_bytes(a.sstride, g.n_groups, g.wide);
    const int blocks = a.rep_list ? a.rep_count : a.R;
    const bool production = sweep_args_are_lean(a) && a.rule == SGA_RULE_METROPOLIS && !a.rep_list;
    void (*kern)(const SweepArgs, const GroupArgs) =
        production ? (rest ? (g.wide ? sweep_groups_kernel<true, true> : sweep_groups_kernel<false, true>)
                           : (g.wide ? sweep_groups_kernel<true, false> : sweep_groups_kernel<false, false>))
                   : (rest ? (g.wide ? sweep_groups_general_kernel<true, true> : sweep_groups_general_kernel<false, true>)
                           : (g.wide ? sweep_groups_general_kernel<true, false> : sweep_groups_general_kernel<false, false>));
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    if (production) {
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(64 * waves), lds, st, a, g);
        if (rest)
            note_sweep_kernel("sweep_groups_kernel<%s sums, stored remainder> x %d wave(s), windows of 128 updates per wave",
                              g.wide ? "int32" : "int16", waves);
        else
            note_sweep_kernel("sweep_groups_kernel<%s sums> x %d wave(s), windows of 128 updates per wave", g.wide ? "int32" : "int16",
                              waves);
    } else {
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds, st, a, g);
        if (rest)
            note_sweep_kernel("sweep_groups_general_kernel<%s sums, stored remainder> x 1 wave, one update at a time",
                              g.wide ? "int32" : "int16");
        else
            note_sweep_kernel("sweep_groups_general_kernel<%s sums> x 1 wave, one update at a time", g.wide ? "int32" : "int16");
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// Full energy: -1/2 fp32(sum_i mv_i s_i) - fp32(h . s), mv_i the fp32 row sum (core/ising_model.py:149-174); X and
// Y in the canonical per-replica order (sga_kernels.h, energy_block_rows).  One workgroup per replica.
// ---------------------------------------------------------------------------------------
template <bool WIDE, bool REST>
__global__ void __launch_bounds__(256) energy_groups_kernel(const EnergyArgs a, const GroupArgs g) {
    using sum_t = typename GroupSums<WIDE>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned int *bits = reinterpret_cast<unsigned int *>(smem);
    sum_t *sums = reinterpret_cast<sum_t *>(smem + a.sstride / 8);
    double *ce = reinterpret_cast<double *>(smem + a.sstride / 8 + (((size_t)g.n_groups * sizeof(sum_t) + 15) & ~(size_t)15));
    double *ch = ce + 4 * ENERGY_MAX_BLOCKS;
    const int tid = threadIdx.x, r = blockIdx.x;
    spins_to_bits(a.spins + (long long)r * a.sstride, bits, a.sstride, tid, 256);
    __syncthreads();
    groups_load_sums(g, bits, sums, tid, 256);
    __syncthreads();
    double X, Y;
    energy_canonical_sums(
        a.n, a.block_rows,
        [&](int i) {
            int si;
            float mv = groups_row_sum(g, bits, sums, i, si);
            if constexpr (REST) mv += groups_rest_row_sum(g, bits, i);
            return (double)mv * (double)si;
        },
        [&](int i) { return (double)a.h[i] * (((bits[i >> 5] >> (i & 31)) & 1u) ? -1.0 : 1.0); }, ce, ch, X, Y);
    if (tid == 0) a.energy[r] = -0.5 * (double)(float)X + (-(double)(float)Y);
}

size_t groups_energy_lds_bytes(int sstride, int n_groups, int wide) {
    const size_t sums = ((size_t)n_groups * (wide ? 4 : 2) + 15) & ~(size_t)15;
    return (size_t)sstride / 8 + sums + 2 * 4 * ENERGY_MAX_BLOCKS * sizeof(double);
}

hipError_t launch_energy_groups(const EnergyArgs &a, const GroupArgs &g, hipStream_t st) {
    const size_t lds = groups_energy_lds_bytes(a.sstride, g.n_groups, g.wide);
    void (*kern)(const EnergyArgs, const GroupArgs) =
        g.rest.nnz > 0 ? (g.wide ? energy_groups_kernel<true, true> : energy_groups_kernel<false, true>)
                       : (g.wide ? energy_groups_kernel<true, false> : energy_groups_kernel<false, false>);
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(a.R), dim3(256), lds, st, a, g);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// Local fields of single sites (IsingModel.get_local_field, core/ising_model.py:176-185), spins read from HBM: one
// wave per requested site, the site's groups one after the other, a group's members across the lanes.
// ---------------------------------------------------------------------------------------
template <bool REST>
__global__ void __launch_bounds__(64) fields_groups_kernel(const GroupArgs g, const int8_t *spins, const float *h,
                                                           const int32_t *sites, double *out) {
    const int lane = threadIdx.x;
    const int site = sites[blockIdx.x];
    const int si = spins[site];
    float acc = 0.0f;
    for (int m = g.gptr[site]; m < g.gptr[site + 1]; ++m) {
        const int2 ent = g.gent[m];
        int s = 0;
        for (long long q = g.member_ptr[ent.x] + lane; q < g.member_ptr[ent.x + 1]; q += 64) s += spins[g.members[q]];
        s = wave_sum(s);
        acc += __int_as_float(ent.y) * (float)(s - si);
    }
    if constexpr (REST) {  // the site's remainder row across the lanes
        float part = 0.0f;
        for (int m = g.rest.rptr[site] + lane; m < g.rest.rptr[site + 1]; m += 64) {
            const int2 ent = g.rest.rent[m];
            part += __int_as_float(ent.y) * (float)spins[ent.x];
        }
        acc += wave_sum(part);
    }
    if (lane == 0) out[blockIdx.x] = (double)acc + (double)h[site];
}

hipError_t launch_fields_groups(const GroupArgs &g, const int8_t *spins, const float *h, const int32_t *sites, int count,
                                double *out, hipStream_t st) {
    if (count <= 0) return hipSuccess;
    if (g.rest.nnz > 0)
        hipLaunchKernelGGL(fields_groups_kernel<true>, dim3(count), dim3(64), 0, st, g, spins, h, sites, out);
    else
        hipLaunchKernelGGL(fields_groups_kernel<false>, dim3(count), dim3(64), 0, st, g, spins, h, sites, out);
    return hipGetLastError();
}

// sum_j |R_ij| per remainder row, in fp64 (the set-time bound adds it to the row's group part on the host)
__global__ void __launch_bounds__(256) groups_rest_row_abs_kernel(const long long *rowptr, const float *val, int n, double *out) {
    const int lane = threadIdx.x & 63;
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int n_waves = (int)((gridDim.x * blockDim.x) >> 6);
    for (int i = wave; i < n; i += n_waves) {
        double acc = 0.0;
        for (long long j = rowptr[i] + lane; j < rowptr[i + 1]; j += 64) acc += (double)fabsf(val[j]);
        acc = wave_sum(acc);
        if (lane == 0) out[i] = acc;
    }
}

hipError_t launch_groups_rest_row_abs(const long long *rowptr, const float *val, int n, double *out, hipStream_t st) {
    const int blocks = (int)std::min<long long>(((long long)n + 3) / 4, 256 * 32);
    hipLaunchKernelGGL(groups_rest_row_abs_kernel, dim3(blocks), dim3(256), 0, st, rowptr, val, n, out);
    return hipGetLastError();
}

}  // namespace sga
