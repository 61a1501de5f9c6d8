// sweep_dense_rs.hip -- "row-shared windows": the dense Metropolis sweep of integer problems with ONE read of a
// coupling row per proposed site and window, instead of one per proposal; the Glauber and heat-bath
// rules walk the same windows (ANYRULE, below).
//
// The sites and uniforms come from the counter RNG (the stream of fetch_pair / PairSource), so every replica's
// proposals are known ahead of the chain.  A sweep is cut into windows of W updates per replica; each window runs
//   * fields: one workgroup per proposed site i takes row i as bit-planes (sign of J, and one plane per binary digit
//     of |J|) and dots it with the window-start spins (bits) of every replica that proposes i inside the window:
//     base(r, t) = sum_j J_ij s_j -- a full row sum of n terms per proposal.  The planes of the whole matrix are made
//     once per problem and stay in HBM (rs_planes_kernel, RowSharedPlan::jp): J does not change between two
//     sga_set_* calls, and a plane row is (planes + 1) / 32 of the fp32 row.  Only int8 rows with 8 magnitude planes,
//     whose planes would outweigh J, are converted on chip per window (rs_fields_kernel).  Over resident planes and
//     long rows the same sums are formed per TILE of consecutive sites, so that a replica's spin bits are read once per
//     tile, not once per proposal, and from sign planes alone where every |J_ij| is 1 (rs_fields_tiles_kernel; option
//     "row_shared_fields");
//   * chain: one wave per replica holds the W pending fields, one per (lane, block of 64 updates), and walks the
//     blocks in order.  A block first takes the corrections -2 J[i_a][i_t] s_a (J symmetric: read from row i_a) of
//     every accept the window has made so far, its spins negated where the site repeats; then its 64 updates are
//     decided at once against the fields as they stand, the couplings of the first few accepting ones to the block
//     are fetched together, and accepts are committed (energy, spin, the block's fields) from registers for as long
//     as the first accepting update is one of those fetched: a memory round trip per batch, not per accept.
// J and h are integer valued with every partial sum below 2^24 (the look-ahead form's proof): the base sums and the
// corrected fields are exactly the fp32 row sums of the one-update-at-a-time chain, the accept rule is the table
// form's, and every decision, energy, spin and counter is bit-identical.  No field outlives its window.
// Many field vectors over ONE matrix (sga_set_dense_shared, a.reps_per_model > 0): plan, fields, planes and corrections
// know J and the replicas' spins only, so they run unchanged -- a (window, site) bucket holds the proposals of every
// replica of every model, and the row is read once for all of them.  h enters in the chain alone: a wave resolves its
// replica's model once and reads that model's h.  The bound above is then asked of the batch: the set-time scan takes
// max (sum_j |J_ij| + |h_mi|) over every model m and site i (a.table_m, one accept table for the batch), so every
// partial sum of every model stays below 2^24 with the batch-wide max of |h|, and each model walks the chain of a
// one-model engine holding (J, h_m) -- whose own, smaller table_m tabulates the same values expf_det(-2 q / T).
// The window plan -- which (replica, update) proposes which site -- is one counting sort per sweep, histogrammed in
// LDS per (window, group of replicas): no atomic of it reaches memory.
//
// GRID (option "row_shared_grid", RowSharedGridPlan::k): J on a binary grid, any finite fp32 h -- the problems
// with table_m == 0 that sga_classify.cpp's row_shared_grid admits.  Every J_ij is an integer multiple of 2^-k (k <=
// 30), |2^k J_ij| <= 255 and B = 2^k max_i sum_j |J_ij| < 2^24.  The planes and jabs are those of the integers 2^k J_ij
// (the scaling is a power-of-two multiply of a value below 2^8: exact), so plan, fields and base are the integer
// form's: base = D = 2^k sum_j J_ij s_j against the window-start spins, an integer with |D| <= B.  Proof that the chain
// is the row kernels':
//   * f = ldexpf((float)D, -k) is exact (|D| < 2^24, and the exponent stays far inside fp32's range: k <= 30).  A
//     correction -2 J[i_a][i_t] s_a is an integer multiple of 2^-k (read as the fp32 J itself, or decoded from one
//     magnitude plane as +-2^-k), and the corrected field is 2^-k times the row sum of 2^k J against the spins as they
//     then stand, again at most B in magnitude.  So every partial sum of the corrected field, in ANY order of the
//     corrections, is 2^-k times an integer below 2^24 (an intermediate state is a spin state too): exact in fp32.
//   * The row kernel's dot for the same spins is the fp32 rounding of the exact row sum -- accumulated in fp64 where
//     the class is f64-exact (every partial sum a multiple of 2^-k below 2^24 / 2^k: exact), in fp32 for integer J
//     with sums below 2^24, in int32 for int8 rows -- and that sum is representable, so dot == the corrected field.
//   * field = (double)dot + (double)h and dE = 2 s field are then formed by metropolis_accept (sweep_common.h) on the
//     row kernels' own arguments: the same decision -- T = 0, T = inf and the 104 T cut-off with it -- and the same
//     dE, and E += dE runs in chain order.  h never enters a sum that has to be exact.
// A shared-coupling batch: k, the planes and the bound are the batch's (one J; the bound's word takes the largest
// |h| of any model), each wave reads its model's h.  The non-GRID instantiations are the integer form's, unchanged:
// the GRID ones take a plan type of their own (RowSharedGridPlan), so not even an argument offset moves in the others.
//
// ANYRULE (a.rule is SGA_RULE_GLAUBER or SGA_RULE_HEAT_BATH): nothing above the chain knows the rule -- every rule takes
// one (site, u) pair per update from the same stream coordinates, so plan, fields, planes and corrections are
// unchanged -- and the chain's block logic needs the decision to be a pure function of (field, spin, u, T) only: the
// first lane that flips is the chain's next flip, every lane before it stays against fields that hold all earlier flips,
// and "flip iff new_spin != s_i" is such a function exactly as "accept" is.  The decision is metropolis_accept(a.rule,
// SGA_ARITH_F64, ...), the row kernels' own (sweep_dense_impl.h), in the integer and the GRID form alike.  Integer form:
// the field stays the exact integer-valued fp32 it is above (every partial sum of the corrected field an integer below
// 2^24, in any order), which is the row kernel's dot for the same spins, so field = (double)dot + (double)h is the row
// kernel's value; GRID: the proof above does not mention the rule.  dE = 2 s field is formed as metropolis_accept
// forms it and E += dE runs in chain order (heat bath too: only the per-update record is negated there, and the form
// keeps none).  Glauber's x = (float)(-2.0 * field / T) keeps its fp64 divide per lane and heat bath's
// x = (float)((-2.0 * (1.0 / T)) * field) its operation sequence (the factor is wave-uniform: formed once, the same
// operations): T = 0, T = inf and a zero field give the row kernels' +-inf, NaN and -+0 and their decisions.
// With ANYRULE off an instantiation is the Metropolis code, unchanged.
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "sweep_common.h"

namespace sga {

// the plan argument of an instantiation, and its parts
template <bool GRID>
using RsPlanArg = typename std::conditional<GRID, RowSharedGridPlan, RowSharedPlan>::type;
__device__ __forceinline__ const RowSharedPlan &rs_plan(const RowSharedPlan &p) { return p; }
__device__ __forceinline__ const RowSharedPlan &rs_plan(const RowSharedGridPlan &g) { return g.p; }
__device__ __forceinline__ int rs_grid_k(const RowSharedPlan &) { return 0; }
__device__ __forceinline__ int rs_grid_k(const RowSharedGridPlan &g) { return g.k; }

// Spin and coupling bits share one layout: element j = 256 g + 4 l + q sits in bit l of 64-bit word 4 g + q (a lane
// that loads four consecutive elements contributes one bit to each of four ballots).
__device__ __forceinline__ void rs_bit_of(int j, int &w32, unsigned int &bit) {
    const int g = j >> 8, e = j & 255, l = e >> 2, q = e & 3;
    w32 = 2 * (4 * g + q) + (l >> 5);
    bit = 1u << (l & 31);
}

// site and uniform bits of update t of sweep k of replica r: fetch_pair's stream
__device__ __forceinline__ void rs_update(const SweepArgs &a, int r, int k, int t, int &site, uint32_t &ubits) {
    const u32x4 w = philox4x32_10((uint32_t)(t >> 1), a.sweep0 + (uint32_t)k, a.replica0 + (uint32_t)r, DOMAIN_SWEEP,
                                  a.seed_lo, a.seed_hi);
    const bool second = t & 1;
    site = (int)word_to_site(second ? w.z : w.x, (uint32_t)a.n);
    ubits = (second ? w.w : w.y) >> 8;
}

// ---- plan: counting sort of the sweep's (replica, update) pairs by (window, site) --------------------------------
// A workgroup owns one slice -- window w, replica group g (2^log_rg replicas) -- and one tile of RS_PLAN_TILE sites:
// its counters are LDS words (64 KiB at most, so any n is served: n <= 16384 is one tile, beyond that every tile
// walks the slice's Philox blocks again and keeps the sites that are its own).  count: histogram -> cnt[w][g][site].
// scan, per window: entries ordered by (site, group) -> off[w][site], and cnt[w][g][site] becomes the first entry of
// (w, g, site).  fill: the same walk, positions handed out from the LDS copy of the slice's cursors.  The order of
// the entries inside a (window, site) bucket is whatever the LDS atomics make it; nothing depends on it (each entry
// names its own base slot).
constexpr int RS_PLAN_TILE = 16384;

template <bool FILL>
__global__ void __launch_bounds__(256) rs_plan_kernel(const SweepArgs a, RowSharedPlan p, int k) {
    extern __shared__ int slot[];  // [min(n, RS_PLAN_TILE)]
    const int g = blockIdx.x, w = blockIdx.y, s0 = blockIdx.z * RS_PLAN_TILE, n = a.n, tid = threadIdx.x;
    const int ns = min(RS_PLAN_TILE, n - s0);
    int *mine = p.cnt + ((long long)w * p.n_groups + g) * n + s0;
    for (int i = tid; i < ns; i += 256) slot[i] = FILL ? mine[i] : 0;
    __syncthreads();
    const int r0 = g << p.log_rg, nr = min(1 << p.log_rg, a.R - r0);
    const int t0 = w << p.log_w, nt = min(p.W, n - t0);  // t0 is even: one Philox block serves updates 2 b, 2 b + 1
    const int lhalf = p.log_w - 1, hmask = (1 << lhalf) - 1;
    for (int x = tid; x < (nr << lhalf); x += 256) {
        const int r = r0 + (x >> lhalf), b = x & hmask;
        if (2 * b >= nt) continue;
        const u32x4 q = philox4x32_10((uint32_t)((t0 >> 1) + b), a.sweep0 + (uint32_t)k, a.replica0 + (uint32_t)r,
                                      DOMAIN_SWEEP, a.seed_lo, a.seed_hi);
        const int sA = (int)word_to_site(q.x, (uint32_t)n) - s0, sB = (int)word_to_site(q.z, (uint32_t)n) - s0;
        const bool inA = (unsigned)sA < (unsigned)ns, inB = 2 * b + 1 < nt && (unsigned)sB < (unsigned)ns;
        if constexpr (FILL) {
            if (inA) p.ent[atomicAdd(&slot[sA], 1)] = (r << p.log_w) | (2 * b);
            if (inB) p.ent[atomicAdd(&slot[sB], 1)] = (r << p.log_w) | (2 * b + 1);
        } else {
            if (inA) atomicAdd(&slot[sA], 1);
            if (inB) atomicAdd(&slot[sB], 1);
        }
    }
    if constexpr (!FILL) {
        __syncthreads();
        for (int i = tid; i < ns; i += 256) mine[i] = slot[i];
    }
}

// The scan, per window: exclusive scan of its counts in (site, group) order, entries of window w start at R w W.  One
// workgroup per (window, chunk of RS_SCAN_CHUNK sites).  totals: the chunk's count over every group -> tot[w][chunk].
constexpr int RS_SCAN_CHUNK = 1024;

__global__ void __launch_bounds__(RS_SCAN_CHUNK) rs_scan_totals_kernel(const SweepArgs a, RowSharedPlan p) {
    __shared__ int part[RS_SCAN_CHUNK / 64];
    const int c = blockIdx.x, w = blockIdx.y, tid = threadIdx.x, n = a.n, G = p.n_groups;
    const int *cnt = p.cnt + (long long)w * G * n;
    const int i = c * RS_SCAN_CHUNK + tid;
    int v = 0;
    if (i < n)
        for (int g = 0; g < G; ++g) v += cnt[(long long)g * n + i];
    v = wave_sum(v);
    if ((tid & 63) == 0) part[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int x = 0; x < RS_SCAN_CHUNK / 64; ++x) t += part[x];
        p.tot[(long long)w * gridDim.x + c] = t;
    }
}

// the scan proper: the chunk's carry is the prefix of the chunk totals (at most ceil(n / RS_SCAN_CHUNK) values)
__global__ void __launch_bounds__(RS_SCAN_CHUNK) rs_scan_kernel(const SweepArgs a, RowSharedPlan p) {
    __shared__ int sh[RS_SCAN_CHUNK];
    const int c = blockIdx.x, w = blockIdx.y, tid = threadIdx.x, n = a.n, G = p.n_groups;
    int *cnt = p.cnt + (long long)w * G * n;
    int *off = p.off + (long long)w * (n + 1);
    const int *tot = p.tot + (long long)w * gridDim.x;
    int carry = a.R * (w << p.log_w);
    for (int x = 0; x < c; ++x) carry += tot[x];
    const int i = c * RS_SCAN_CHUNK + tid;
    int v = 0;
    if (i < n)
        for (int g = 0; g < G; ++g) v += cnt[(long long)g * n + i];
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < RS_SCAN_CHUNK; d <<= 1) {  // inclusive Hillis-Steele scan
        const int x = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += x;
        __syncthreads();
    }
    if (i < n) {
        int run = carry + sh[tid] - v;
        off[i] = run;
        for (int g = 0; g < G; ++g) {
            const int cc = cnt[(long long)g * n + i];
            cnt[(long long)g * n + i] = run;
            run += cc;
        }
    }
    if (c == (int)gridDim.x - 1 && tid == 0) off[n] = carry + sh[RS_SCAN_CHUNK - 1];
}

// int8 spins -> the bit layout above (1 = spin down); one workgroup per replica
__global__ void __launch_bounds__(256) rs_pack_kernel(const SweepArgs a, RowSharedPlan p) {
    const int r = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nseg = (a.n + 255) >> 8;
    const int8_t *src = a.spins + (long long)r * a.sstride;
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(p.bits) + (long long)r * (p.nw32 / 2);
    for (int g = wv; g < nseg; g += 4) {
        const int e = 256 * g + 4 * lane;
        const unsigned int v = e < a.n ? *reinterpret_cast<const unsigned int *>(src + e) : 0u;  // (pad spins are 0)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned long long m = ballot64(((v >> (8 * q + 7)) & 1u) != 0u);
            if (lane == 0) dst[4 * g + q] = m;
        }
    }
}

// ---- the tile kernel's plan: the sweep's pairs sorted by (window, slice of rg replicas, tile, replica) ----------------
// The tile kernel needs the entries of its S sites grouped by replica, and no order by site: so a workgroup owns one slice
// (window w, replicas r0 .. r0 + rg), sorts the slice's entries in LDS by (tile, replica in the slice) -- a counting sort:
// count per key while the Philox blocks are walked, the sites kept in registers; scan; place -- and writes the sorted
// slice out in one piece, consecutive lanes to consecutive words, at its fixed place R t0 + r0 nt of ent[] (the regions
// tile ent[] exactly).  One launch per sweep, no atomic and no partial line of entries reaches memory.  The entries of a
// (slice, tile) pair are a contiguous run, ordered by replica; the run's first entry (relative to the slice, 16 bits)
// goes to runs[w][tile][slice], in the by-site plan's cnt allocation (row_shared_tile_plan_runs_fit), so that a tile reads
// the bounds of its runs over all slices as two contiguous rows (the last tile's runs end with their slices).
// The entry word: site - tile S (12 bits: S <= RS_TILE_MAX_SITES) | replica - r0 (5 bits) << 12 | update in the window
// << 17; the reader knows the slice from the run it reads.  The order inside a (tile, replica) bucket is whatever the LDS
// atomics make it; every entry names its own base slot.
// blockIdx.z: the range of tpp tiles this workgroup sorts (row_shared_tile_plan: one range wherever the counters of all
// tiles fit); a range walks all of the slice's blocks, counts the entries of earlier tiles -- its place in the slice --
// and drops those of later ones.
constexpr int RS_TILE_PLAN_PAIRS = 32 * 1024 / 2 / RS_TILE_PLAN_THREADS;  // Philox blocks per thread: rg W <= 32 * 1024

// site / S without a divide: mul = ceil(2^32 / S), S >= 2; the product's high word is the quotient or one above it
__device__ __forceinline__ int rs_tile_of(int site, int S, unsigned int mul, int &ls) {
    int tile = (int)__umulhi((unsigned int)site, mul);
    ls = site - tile * S;
    if (ls < 0) --tile, ls += S;
    return tile;
}

__global__ void __launch_bounds__(RS_TILE_PLAN_THREADS) rs_tile_plan_kernel(const SweepArgs a, RowSharedPlan p, int k, int S,
                                                                           int log_trg, int tpp) {
    constexpr int T = RS_TILE_PLAN_THREADS, NP = RS_TILE_PLAN_PAIRS;
    extern __shared__ int stage[];  // [rg W] the sorted entries, [tpp rg] counters then cursors, RS_TILE_PLAN_EXTRA words
    const int sl = blockIdx.x, w = blockIdx.y, n = a.n, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int rg = 1 << log_trg, r0 = sl << log_trg, nr = min(rg, a.R - r0);
    const int t0 = w << p.log_w, nt = min(p.W, n - t0);  // t0 is even: one Philox block serves updates 2 b, 2 b + 1
    const int ntiles = (n + S - 1) / S, tl0 = blockIdx.z * tpp, ntl = min(tpp, ntiles - tl0), ncnt = ntl << log_trg;
    int *cnt = stage + (rg << p.log_w), *wtot = cnt + (tpp << log_trg), *sums = wtot + T / 64;  // sums: [0] earlier tiles, [1] ours
    const unsigned int mul = 0xffffffffu / (unsigned int)S + 1u;
    for (int c = tid; c < ncnt; c += T) cnt[c] = 0;
    if (tid < 2) sums[tid] = 0;
    __syncthreads();
    const int lhalf = p.log_w - 1, hmask = (1 << lhalf) - 1, np = nr << lhalf;
    int site[2 * NP];  // the sites of this thread's updates that fall into the range; -1: none
    int below = 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int x = tid + j * T, rr = x >> lhalf, b = x & hmask;
        site[2 * j] = site[2 * j + 1] = -1;
        if (x < np && 2 * b < nt) {
            const u32x4 q = philox4x32_10((uint32_t)((t0 >> 1) + b), a.sweep0 + (uint32_t)k, a.replica0 + (uint32_t)(r0 + rr),
                                          DOMAIN_SWEEP, a.seed_lo, a.seed_hi);
            const int sA = (int)word_to_site(q.x, (uint32_t)n), sB = 2 * b + 1 < nt ? (int)word_to_site(q.z, (uint32_t)n) : -1;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int s = h ? sB : sA;
                if (s < 0) continue;
                int ls;
                const int tl = rs_tile_of(s, S, mul, ls) - tl0;
                if (tl < 0) ++below;
                else if (tl < ntl) {
                    atomicAdd(&cnt[(tl << log_trg) + rr], 1);
                    site[2 * j + h] = s;
                }
            }
        }
    }
    if (tl0 > 0) {  // (workgroup-uniform)
        below = wave_sum(below);
        if (lane == 0 && below) atomicAdd(&sums[0], below);
    }
    __syncthreads();
    below = sums[0];
    {  // exclusive scan of cnt in (tile, replica) order: thread t owns counters [t per, (t + 1) per)
        const int per = (ncnt + T - 1) / T, c0 = tid * per;
        int sum = 0;
        for (int j = 0; j < per; ++j)
            if (c0 + j < ncnt) sum += cnt[c0 + j];
        int inc = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wtot[wv] = inc;
        __syncthreads();
        int run = inc - sum;
        for (int x = 0; x < wv; ++x) run += wtot[x];
        unsigned short *runs = reinterpret_cast<unsigned short *>(p.cnt) + ((long long)w * ntiles + tl0) * gridDim.x + sl;
        for (int j = 0; j < per; ++j)
            if (c0 + j < ncnt) {
                const int c = cnt[c0 + j];
                cnt[c0 + j] = run;
                if (((c0 + j) & (rg - 1)) == 0) runs[(long long)((c0 + j) >> log_trg) * gridDim.x] = (unsigned short)(below + run);
                run += c;
            }
        if (tid == T - 1) sums[1] = run;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int x = tid + j * T, rr = x >> lhalf, b = x & hmask;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int s = site[2 * j + h];
            if (s < 0) continue;
            int ls;
            const int tl = rs_tile_of(s, S, mul, ls) - tl0;
            stage[atomicAdd(&cnt[(tl << log_trg) + rr], 1)] = ls | (rr << 12) | ((2 * b + h) << 17);
        }
    }
    __syncthreads();
    int *dst = p.ent + (long long)a.R * t0 + (long long)r0 * nt + below;
    for (int i = tid, m = sums[1]; i < m; i += T) dst[i] = stage[i];
}

// ---- a row of J as bit-planes ------------------------------------------------------------------------------------
// PL magnitude planes: |J| < 2^PL.  planes: [PL + 1][nw = 4 nseg] 64-bit words (sign plane first), in LDS or in the
// resident copy; every word is written.  Called by a workgroup of four waves; returns this lane's share of sum |J_ij|.
// GRID: the planes of 2^gk J (fp32 rows on the grid 2^-gk: every scaled element an integer, the multiply exact).
template <typename JE, int PL, bool GRID>
__device__ __forceinline__ int rs_row_to_planes(const JE *row, int n, unsigned long long *planes, int lane, int wv, int gk) {
    const int nseg = (n + 255) >> 8, nw = 4 * nseg;
    int absum = 0;
    // four segments per wave in flight, then their ballots
    for (int g0 = wv; g0 < nseg; g0 += 16) {
        int v[4][4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int e = 256 * (g0 + 4 * s) + 4 * lane;  // e < n <= ldj, e % 4 == 0: the 4-element load stays in the row
            if (g0 + 4 * s < nseg && e < n) {
                if constexpr (std::is_same<JE, float>::value) {
                    float4 x = *reinterpret_cast<const float4 *>(row + e);
                    if constexpr (GRID) x.x = ldexpf(x.x, gk), x.y = ldexpf(x.y, gk), x.z = ldexpf(x.z, gk), x.w = ldexpf(x.w, gk);
                    v[s][0] = (int)x.x, v[s][1] = (int)x.y, v[s][2] = (int)x.z, v[s][3] = (int)x.w;
                } else {
                    const int x = *reinterpret_cast<const int *>(row + e);
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[s][q] = (int)(int8_t)(x >> (8 * q));
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[s][q] = 0;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (e + q >= n) v[s][q] = 0;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int g = g0 + 4 * s;
            if (g >= nseg) break;  // wave-uniform
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = v[s][q] < 0 ? -v[s][q] : v[s][q];
                absum += m;
                const unsigned long long sg = ballot64(v[s][q] < 0);
                unsigned long long pb[PL];
#pragma unroll
                for (int b = 0; b < PL; ++b) pb[b] = ballot64(((m >> b) & 1) != 0);
                if (lane == 0) {
                    planes[4 * g + q] = sg;
#pragma unroll
                    for (int b = 0; b < PL; ++b) planes[(long long)(1 + b) * nw + 4 * g + q] = pb[b];
                }
            }
        }
    }
    return absum;
}

// the resident copy: one workgroup per row, once per problem
template <typename JE, int PL>
__global__ void __launch_bounds__(256) rs_planes_kernel(const JE *J, long long ldj, int n, unsigned long long *jp, int *jabs) {
    __shared__ int csum[4];
    const int i = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nw = 4 * ((n + 255) >> 8);
    int absum = rs_row_to_planes<JE, PL, false>(J + (long long)i * ldj, n, jp + (long long)i * (PL + 1) * nw, lane, wv, 0);
    absum = wave_sum(absum);
    if (lane == 0) csum[wv] = absum;
    __syncthreads();
    if (threadIdx.x == 0) jabs[i] = csum[0] + csum[1] + csum[2] + csum[3];
}
// GRID: the planes and jabs of 2^gk J (fp32 rows)
template <int PL>
__global__ void __launch_bounds__(256) rs_planes_grid_kernel(const float *J, long long ldj, int n, unsigned long long *jp, int *jabs,
                                                             int gk) {
    __shared__ int csum[4];
    const int i = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nw = 4 * ((n + 255) >> 8);
    int absum = rs_row_to_planes<float, PL, true>(J + (long long)i * ldj, n, jp + (long long)i * (PL + 1) * nw, lane, wv, gk);
    absum = wave_sum(absum);
    if (lane == 0) csum[wv] = absum;
    __syncthreads();
    if (threadIdx.x == 0) jabs[i] = csum[0] + csum[1] + csum[2] + csum[3];
}

// ---- fields from the resident planes: one workgroup (4 waves) per proposed site ------------------------------------
// The site's plane row (PL + 1 planes of nw words) goes to LDS as it is; then a quarter wave (16 lanes, one DPP row) per
// entry: each lane takes two words at a time of the replica's spin bits, and four row-local DPP steps close the sum,
// so a wave finishes four entries per pass.  sum_j J_ij s_j = C - 2 sum_b 2^b popcount(plane_b & (sign ^ spin bits)).
template <int PL>
__global__ void __launch_bounds__(256) rs_fields_planes_kernel(const SweepArgs a, RowSharedPlan p, int win) {
    const int i = blockIdx.x, n = a.n;
    const int *off = p.off + (long long)win * (n + 1);
    const int lo = off[i], hi = off[i + 1];
    if (lo == hi) return;  // nobody proposes this site in this window: the row is not read
    extern __shared__ ulonglong2 prow[];  // [PL + 1][nw / 2]
    const int nw2 = p.nw32 >> 2;           // pairs of 64-bit words per plane (nw is a multiple of 4)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, sub = lane >> 4, l16 = lane & 15;
    const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(p.jp) + (long long)i * (PL + 1) * nw2;
    for (int c = tid; c < (PL + 1) * nw2; c += 256) prow[c] = src[c];
    const int C = p.jabs[i];  // sum_j |J_ij|
    __syncthreads();
    const ulonglong2 *bits = reinterpret_cast<const ulonglong2 *>(p.bits);
    const int wmask = (1 << p.log_w) - 1;
    for (int x0 = lo + 4 * wv; x0 < hi; x0 += 16) {  // wave-uniform bounds: the DPP steps run with every lane on
        const int x = x0 + sub;
        const bool live = x < hi;
        const int e = p.ent[live ? x : lo];
        const ulonglong2 *s = bits + (long long)(e >> p.log_w) * nw2;
        int acc = 0;
        for (int c = l16; c < nw2; c += 16) {
            const ulonglong2 sv = s[c], sg = prow[c];
            const unsigned long long x0w = sv.x ^ sg.x, x1w = sv.y ^ sg.y;
#pragma unroll
            for (int b = 0; b < PL; ++b) {
                const ulonglong2 pb = prow[(1 + b) * nw2 + c];
                acc += (__popcll(pb.x & x0w) + __popcll(pb.y & x1w)) << b;
            }
        }
        acc += dpp_move<DPP_QUAD_XOR1>(acc);
        acc += dpp_move<DPP_QUAD_XOR2>(acc);
        acc += dpp_move<DPP_ROW_HALF_MIRROR>(acc);
        acc += dpp_move<DPP_ROW_MIRROR>(acc);
        if (live && l16 == 0) p.base[(long long)(e >> p.log_w) * p.W + (e & wmask)] = C - 2 * acc;
    }
}

// ---- fields from the resident planes in tiles: one workgroup (16 waves) per tile of S consecutive sites ---------------
// The per-site kernel reads a replica's spin bits from L2 once per ENTRY; a replica proposes about W S / n sites of a
// tile inside a window, so a workgroup that owns the tile needs them once per replica.  The tile's entries are the
// concatenation, in slice order, of its runs in the tile plan (rs_tile_plan_kernel): grouped by replica as they stand,
// each carrying its site's index in the tile, so the kernel sorts nothing -- a prefix over the runs' lengths, then a
// coalesced copy to LDS (a range longer than the entry buffer goes through in chunks: successive ranges of the
// concatenation, cut wherever they fall).  The plane rows of the tile go to LDS beside the copy.
// Then the per-site kernel's inner loop: the entries of a replica sit in adjacent quarter waves and passes, so their
// spin-bit loads merge or hit L1.  The order inside a replica's run is the plan's; every entry names its own base slot.
// ONES (every off-diagonal |J_ij| is 1: the magnitude plane is all ones but for the diagonal and the pad): the rows
// are their sign planes alone.  sum_j |J_ij| [sign_ij != spin_j] = popcount(sign ^ spin) - spin_i, as the diagonal's sign
// bit is 0 (its term is the spin bit itself, and the magnitude plane would have masked it) and the pad bits are 0 in
// both; base = C - 2 acc as before.
// 16 bytes of a row against 16 bytes of spin bits: sum_b 2^b popcount(plane_b & (sign ^ spin)); ONES: popcount(sign ^ spin)
template <int PL, bool ONES>
__device__ __forceinline__ int rs_tile_word(const ulonglong2 sv, const ulonglong2 *row, int nw2, int c) {
    const ulonglong2 sg = row[c];
    const unsigned long long x0w = sv.x ^ sg.x, x1w = sv.y ^ sg.y;
    if constexpr (ONES) {
        return __popcll(x0w) + __popcll(x1w);
    } else {
        int acc = 0;
#pragma unroll
        for (int b = 0; b < PL; ++b) {
            const ulonglong2 pb = row[(1 + b) * nw2 + c];
            acc += (__popcll(pb.x & x0w) + __popcll(pb.y & x1w)) << b;
        }
        return acc;
    }
}

// The inner loop of the tile kernel over one sorted chunk.  A quarter wave takes a contiguous piece of the chunk -- the
// four pieces of a wave are equally long, so no quarter wave idles -- and keeps the spin bits of the piece's current
// replica in registers, NK words of 16 bytes per lane (NK = ceil(nw2 / 16), chosen wave-uniformly by the caller, so the
// loads of a replica and the LDS reads of an entry are NK independent instructions without a branch between them; the
// lanes of the last, partial group read word 0 and drop the sum): the bits are read once per replica and piece, about
// once per replica and tile.  NK = 0: longer rows stream the bits per entry, as the per-site kernel
// does (from L1 now, a replica's entries being adjacent).
struct RsTileChunk {
    const int *sent;
    const unsigned short *sls;
    const int *sjabs;
    const ulonglong2 *prow, *bits;
    int *base;
    int cn, nw2, rw2, log_w, W, nwaves;
};
// The entry loop's addresses as unsigned 32-bit byte offsets beside wave-uniform base pointers (the chain's voff): a
// replica's spin bits at r * 16 nw2 of bits, the entry's slot at 4 e of base (W = 2^log_w, so r W + t is the entry word
// itself), the site's row at ls * 16 rw2 of the LDS image -- 24-bit multiplies; and the next pass's entry read one pass
// ahead.  -DSGA_RS_TILES_LEAN=0: 64-bit pointers formed per entry, the entry read where it is used, as it was.  The bounds (launch_sweep_dense_rs refuses anything beyond them): r < 4096 =
// RS_TILE_MAX_REPLICAS, 16 nw2 < 2^18 (two rows fit LDS) -- bits spans R * 16 nw2 < 2^30 bytes; base spans 4 R W <= 2^24
// bytes (W <= 1024); ls < 2^12 and 16 rw2 < 2^18, their product inside LDS.
#ifndef SGA_RS_TILES_LEAN
#define SGA_RS_TILES_LEAN 1
#endif
constexpr bool RS_TILES_LEAN = SGA_RS_TILES_LEAN != 0;
// The tile kernel's prologue with every independent load issued before the first wait ("Tile prologue"):
// the run bounds read once and kept across the barrier, the row constants and plane rows loaded at kernel entry and
// stored to LDS behind the prefix, the entries copied flat -- four dependent trips to memory before the first popcount
// (bounds with rows; entries; own spin bits; the first replica's bits), whatever S and the number of runs.
// -DSGA_RS_TILES_PROLOGUE=0: a wave per row and per run, each load behind its own wait, as it was.
#ifndef SGA_RS_TILES_PROLOGUE
#define SGA_RS_TILES_PROLOGUE 1
#endif
constexpr bool RS_TILES_PROLOGUE = SGA_RS_TILES_PROLOGUE != 0;

template <int PL, bool ONES, int NK>
__device__ __forceinline__ void rs_tile_pieces(const RsTileChunk &ch, int wv, int sub, int l16) {
    const int L = (ch.cn + 4 * ch.nwaves - 1) / (4 * ch.nwaves), x1 = (4 * wv + sub) * L, wmask = (1 << ch.log_w) - 1;
    constexpr int NR = NK > 0 ? NK : 1;
    const int clast = l16 + 16 * (NR - 1);
    const bool vlast = clast < ch.nw2;
    const int cl = vlast ? clast : 0;
    ulonglong2 sv[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) sv[k] = make_ulonglong2(0ull, 0ull);
    int rcur = -1;
    if constexpr (RS_TILES_LEAN) {
        const char *bitsb = reinterpret_cast<const char *>(ch.bits), *prowb = reinterpret_cast<const char *>(ch.prow);
        char *baseb = reinterpret_cast<char *>(ch.base);
        const unsigned int rowb = 16u * (unsigned int)ch.nw2, lrowb = 16u * (unsigned int)ch.rw2;
        const unsigned int o16 = 16u * (unsigned int)l16, ocl = 16u * (unsigned int)cl;
        // (the entry of the next pass is read from LDS under this one's work: one LDS round trip less on every pass's path)
        bool live_n = x1 < ch.cn;
        unsigned int e_n = (unsigned int)ch.sent[live_n ? x1 : 0], lsd_n = ch.sls[live_n ? x1 : 0];
        for (int t = 0; t < L; ++t) {  // wave-uniform bounds: the DPP steps run with every lane on
            const bool live = live_n;
            const unsigned int e = e_n, lsd = lsd_n, ls = lsd & 0x7fffu;
            const int xn = x1 + t + 1;
            live_n = xn < ch.cn;
            e_n = (unsigned int)ch.sent[live_n ? xn : 0], lsd_n = ch.sls[live_n ? xn : 0];
            const int r = (int)(e >> ch.log_w);
            const unsigned int bo = __umul24((unsigned int)r, rowb);  // < 2^30: R <= 4096, 16 nw2 < 2^18
            const ulonglong2 *row = reinterpret_cast<const ulonglong2 *>(prowb + __umul24(ls, lrowb));
            int acc = 0;
            if constexpr (NK > 0) {
                if (live && r != rcur) {  // a new run
                    rcur = r;
                    const char *s = bitsb + (size_t)(bo + o16);
#pragma unroll
                    for (int k = 0; k < NK - 1; ++k) sv[k] = *reinterpret_cast<const ulonglong2 *>(s + 256 * k);
                    sv[NK - 1] = *reinterpret_cast<const ulonglong2 *>(bitsb + (size_t)(bo + ocl));
                }
#pragma unroll
                for (int k = 0; k < NK - 1; ++k) acc += rs_tile_word<PL, ONES>(sv[k], row, ch.nw2, l16 + 16 * k);
                const int last = rs_tile_word<PL, ONES>(sv[NK - 1], row, ch.nw2, cl);
                acc += vlast ? last : 0;
            } else {
                for (int c = l16; c < ch.nw2; c += 16)
                    acc += rs_tile_word<PL, ONES>(*reinterpret_cast<const ulonglong2 *>(bitsb + (size_t)(bo + 16u * (unsigned int)c)), row,
                                                  ch.nw2, c);
            }
            acc += dpp_move<DPP_QUAD_XOR1>(acc);
            acc += dpp_move<DPP_QUAD_XOR2>(acc);
            acc += dpp_move<DPP_ROW_HALF_MIRROR>(acc);
            acc += dpp_move<DPP_ROW_MIRROR>(acc);
            // ONES, the diagonal: its sign bit is 0, so the xor held the replica's own spin bit at site i (lsd >> 15)
            if (live && l16 == 0)  // 4 e < 2^24: e < R W <= 4096 * 1024
                *reinterpret_cast<int *>(baseb + (size_t)(e << 2)) = ch.sjabs[ls] - 2 * (acc - (int)(lsd >> 15));
        }
        return;
    }
    for (int t = 0; t < L; ++t) {  // wave-uniform bounds: the DPP steps run with every lane on
        const int x = x1 + t;
        const bool live = x < ch.cn;
        const int e = ch.sent[live ? x : 0], lsd = ch.sls[live ? x : 0], ls = lsd & 0x7fff, r = e >> ch.log_w;
        const ulonglong2 *s = ch.bits + (long long)r * ch.nw2;
        const ulonglong2 *row = ch.prow + ls * ch.rw2;
        int acc = 0;
        if constexpr (NK > 0) {
            if (live && r != rcur) {  // a new run
                rcur = r;
#pragma unroll
                for (int k = 0; k < NK - 1; ++k) sv[k] = s[l16 + 16 * k];
                sv[NK - 1] = s[cl];
            }
#pragma unroll
            for (int k = 0; k < NK - 1; ++k) acc += rs_tile_word<PL, ONES>(sv[k], row, ch.nw2, l16 + 16 * k);
            const int last = rs_tile_word<PL, ONES>(sv[NK - 1], row, ch.nw2, cl);
            acc += vlast ? last : 0;
        } else {
            for (int c = l16; c < ch.nw2; c += 16) acc += rs_tile_word<PL, ONES>(s[c], row, ch.nw2, c);
        }
        acc += dpp_move<DPP_QUAD_XOR1>(acc);
        acc += dpp_move<DPP_QUAD_XOR2>(acc);
        acc += dpp_move<DPP_ROW_HALF_MIRROR>(acc);
        acc += dpp_move<DPP_ROW_MIRROR>(acc);
        // ONES, the diagonal: its sign bit is 0, so the xor held the replica's own spin bit at site i (lsd >> 15)
        if (live && l16 == 0) ch.base[(long long)r * ch.W + (e & wmask)] = ch.sjabs[ls] - 2 * (acc - (lsd >> 15));
    }
}

template <int PL, bool ONES>
__global__ void __launch_bounds__(RS_TILE_THREADS) rs_fields_tiles_kernel(const SweepArgs a, RowSharedPlan p, int S, int log_trg,
                                                                         int win) {
    constexpr int RP = ONES ? 1 : PL + 1, T = RS_TILE_THREADS, NW = T / 64;
    const int n = a.n, R = a.R, tile0 = blockIdx.x * S, ns = min(S, n - tile0);
    extern __shared__ ulonglong2 prow[];  // [S][RP][nw / 2], then the arrays below (row_shared_tile_lds)
    const int nw2 = p.nw32 >> 2, rw2 = RP * nw2;
    int *sent = reinterpret_cast<int *>(prow + (size_t)S * rw2);  // [RS_TILE_ENTRIES] the chunk's entries by replica
    int *spre = sent + RS_TILE_ENTRIES;                           // [R] entries of the tile before each slice's run (slices <= R)
    int *sjabs = spre + R + S + 1;                                // [S] sum_j |J_ij| (behind S + 1 words the by-site plan's offsets took)                                    // [S] sum_j |J_ij|
    int *wtot = sjabs + S;                                        // [NW] the scan's wave totals
    unsigned short *sls = reinterpret_cast<unsigned short *>(wtot + NW);  // [RS_TILE_ENTRIES] site - tile0 of sent[.] (15 bits)
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), sub = lane >> 4, l16 = lane & 15;
    // the tile's runs, one per slice (rs_tile_plan_kernel): run s is run0[s] ... run1[s] of the slice's region of ent[]
    const int nsl = (R + (1 << log_trg) - 1) >> log_trg, t0 = win << p.log_w, nt = min(p.W, n - t0);
    const bool last = blockIdx.x + 1 == gridDim.x;
    const unsigned short *run0 = reinterpret_cast<const unsigned short *>(p.cnt) + ((long long)win * gridDim.x + blockIdx.x) * nsl;
    const unsigned short *run1 = run0 + nsl;  // (the last tile's runs end where their slices end)
    int total;
    // PROLOGUE: what the loads below fill, kept in registers until the prefix is known (the stores follow the barrier)
    constexpr int NJB = RS_TILE_MAX_SITES / T;                                                     // jabs words per thread
    constexpr int NPW = (int)((RS_TILE_LDS_BUDGET - 6 * RS_TILE_ENTRIES) / 16 + T - 1) / T;        // 16-byte plane words per thread
    constexpr int NEN = RS_TILE_ENTRIES / T;                                                       // entries of a chunk per thread
    const int npw = ns * rw2;  // the image's words: S rw2 16 <= RS_TILE_LDS_BUDGET less the entry buffer, so npw <= NPW T
    // the run starts less the prefix, beside spre where the words are free (a slice of one replica and R > S + 1: not)
    const bool have_sd = 2 * nsl <= R + S + 1;
    int *sd = spre + nsl;
    int st1 = 0, jb[NJB], li[NPW];
    ulonglong2 pw[NPW];
    {  // spre: the exclusive prefix of the runs' lengths, thread t owns slices [t per, (t + 1) per)
        const int per = (nsl + T - 1) / T, s0 = tid * per;
        int sum = 0;
        int en1 = 0;
        if (RS_TILES_PROLOGUE && per == 1) {  // the bounds once, every lane a valid address; then everything else the tile reads
            const unsigned short *end1 = last ? run0 : run1;
            const int s1 = min(tid, nsl - 1);
            st1 = run0[s1];
            en1 = end1[s1];
        }
        if constexpr (RS_TILES_PROLOGUE) {
            // The tile's row constants and plane rows: addresses of the block index alone, the image's words dealt flat to the
            // threads (word c is word c % rw2 of row c / rw2), all of a thread's loads in flight beside the bounds -- the guards
            // are wave-uniform and the lanes past the end read the last word.
#pragma unroll
            for (int j = 0; j < NJB; ++j) {
                jb[j] = 0;
                if (j * T < ns) jb[j] = p.jabs[tile0 + min(tid + j * T, ns - 1)];
            }
            const ulonglong2 *jp2 = reinterpret_cast<const ulonglong2 *>(p.jp) + (long long)tile0 * (PL + 1) * nw2;
            const unsigned int mul = 0xffffffffu / (unsigned int)rw2 + 1u;  // (rw2 >= 2: nw2 is even)
#pragma unroll
            for (int j = 0; j < NPW; ++j) {
                pw[j] = make_ulonglong2(0ull, 0ull);
                li[j] = -1;
                if (j * T < npw) {
                    const int c = tid + j * T;
                    int col;
                    const int s = rs_tile_of(min(c, npw - 1), rw2, mul, col);
                    pw[j] = jp2[(long long)s * ((PL + 1) * nw2) + col];  // (ONES: the sign plane, the first)
                    li[j] = c < npw ? c : -1;
                }
            }
        }
        if (RS_TILES_PROLOGUE && per == 1) {
            const int len = (last ? min(1 << log_trg, R - (tid << log_trg)) * nt : en1) - st1;
            sum = tid < nsl ? len : 0;
        } else {
            for (int j = 0; j < per; ++j)
                if (s0 + j < nsl) sum += (last ? min(1 << log_trg, R - ((s0 + j) << log_trg)) * nt : (int)run1[s0 + j]) - (int)run0[s0 + j];
        }
        int inc = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wtot[wv] = inc;
        __syncthreads();
        int run = inc - sum;
        total = 0;
        for (int w = 0; w < NW; ++w) {
            if (w < wv) run += wtot[w];
            total += wtot[w];
        }
        if (total == 0) return;  // nobody proposes a site of this tile in this window (workgroup-uniform)
        if (RS_TILES_PROLOGUE && per == 1) {
            if (tid < nsl) {
                spre[tid] = run;
                if (have_sd) sd[tid] = st1 - run;
            }
        } else {
            for (int j = 0; j < per; ++j)
                if (s0 + j < nsl) {
                    const int b = run0[s0 + j];
                    spre[s0 + j] = run;
                    if (RS_TILES_PROLOGUE && have_sd) sd[s0 + j] = b - run;
                    run += (last ? min(1 << log_trg, R - ((s0 + j) << log_trg)) * nt : (int)run1[s0 + j]) - b;
                }
        }
    }
    // The plane rows of the whole tile, beside the copy below.  (Reading only the rows somebody proposes was measured
    // against this at 8 replicas, where most rows of a tile go unproposed: the rows come from L2, and marking them during
    // the copy puts their loads behind it and a barrier more -- slower)
    if constexpr (RS_TILES_PROLOGUE) {
#pragma unroll
        for (int j = 0; j < NJB; ++j)
            if (j * T < ns && tid + j * T < ns) sjabs[tid + j * T] = jb[j];
#pragma unroll
        for (int j = 0; j < NPW; ++j)
            if (j * T < npw && li[j] >= 0) prow[li[j]] = pw[j];
    } else {
        for (int s = tid; s < ns; s += T) sjabs[s] = p.jabs[tile0 + s];
        for (int s = wv; s < ns; s += NW) {  // a wave per row
            const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(p.jp) + (long long)(tile0 + s) * (PL + 1) * nw2;
            for (int c = lane; c < rw2; c += 64) prow[s * rw2 + c] = src[c];  // (ONES: the sign plane, the first)
        }
    }
    const ulonglong2 *bits = reinterpret_cast<const ulonglong2 *>(p.bits);
    const int *went = p.ent + (long long)R * t0;  // the window's entries
    const int btop = nsl > 1 ? 1 << (31 - __clz(nsl - 1)) : 0;  // the bisection's first step: the highest bit of nsl - 1
    for (int c0 = 0; c0 < total; c0 += RS_TILE_ENTRIES) {
        const int cn = min(RS_TILE_ENTRIES, total - c0);
        __syncthreads();  // (spre; and the last chunk's readers of sent are ahead of its writers)
        if constexpr (RS_TILES_PROLOGUE) {
            // The chunk is entries c0 ... c0 + cn of the runs' concatenation in slice order -- slices are ascending, disjoint
            // replica ranges and a run is ordered by replica, so it is grouped by replica as it stands.  Flat: thread t takes
            // entries c0 + t + j T and finds the run of each -- the last slice whose prefix is not beyond the entry (empty
            // runs share their prefix with the run behind them) -- by bisecting spre[] in LDS, every step a read of all its
            // entries.  Then the stages, each issued for all of a thread's entries before the next one's first wait: the
            // entry words; ONES: the replica's own spin bit at the site; the LDS stores.  The guards are wave-uniform, and
            // a lane past the chunk's end reads the chunk's last entry and stores nothing.
            int g[NEN], sl[NEN], v[NEN];
            unsigned int ob[NEN];
#pragma unroll
            for (int j = 0; j < NEN; ++j) g[j] = min(c0 + tid + j * T, c0 + cn - 1), sl[j] = 0;
            for (int b = btop; b; b >>= 1) {
#pragma unroll
                for (int j = 0; j < NEN; ++j) {
                    const int m = sl[j] + b;
                    if (spre[min(m, nsl - 1)] <= g[j] && m < nsl) sl[j] = m;
                }
            }
            const int w0 = c0 + 64 * wv;  // the wave's first entry of round 0
#pragma unroll
            for (int j = 0; j < NEN; ++j) {
                v[j] = 0;
                if (w0 + j * T < c0 + cn) {
                    const int d = have_sd ? sd[sl[j]] : (int)run0[sl[j]] - spre[sl[j]];
                    v[j] = went[((sl[j] << log_trg) * nt + d) + g[j]];  // (inside the window's R nt entries)
                }
            }
            if constexpr (ONES) {  // the replica's own spin bit at the site rides in bit 15
#pragma unroll
                for (int j = 0; j < NEN; ++j) {
                    ob[j] = 0u;
                    if (w0 + j * T < c0 + cn) {
                        int w32;
                        unsigned int bit;
                        rs_bit_of(tile0 + (v[j] & 0xfff), w32, bit);
                        const int r = (sl[j] << log_trg) + ((v[j] >> 12) & 31);
                        ob[j] = p.bits[(long long)r * p.nw32 + w32];  // (the word as loaded: masking it here would wait here)
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < NEN; ++j)
                if (w0 + j * T < c0 + cn && c0 + tid + j * T < c0 + cn) {
                    const int r = (sl[j] << log_trg) + ((v[j] >> 12) & 31);
                    int ls = v[j] & 0xfff;
                    if constexpr (ONES) {
                        int w32;
                        unsigned int bit;
                        rs_bit_of(tile0 + ls, w32, bit);
                        if (ob[j] & bit) ls |= 0x8000;
                    }
                    sent[tid + j * T] = (r << p.log_w) | (v[j] >> 17);
                    sls[tid + j * T] = (unsigned short)ls;
                }
        } else {
            // The chunk is entries c0 ... c0 + cn of the runs' concatenation in slice order -- slices are ascending, disjoint
            // replica ranges and a run is ordered by replica, so it is grouped by replica as it stands: a wave per run copies
            // what the chunk holds of it, consecutive lanes consecutive entries.  A wave takes runs wv, wv + NW, ...: it reads
            // the bounds of 64 of them at once, a lane each, so that a run costs one trip to memory, not two in a row.
            for (int sb = wv; sb < nsl; sb += 64 * NW) {
                const int sm = sb + NW * lane;
                int st = 0, b0 = 0, b1 = 0;
                if (sm < nsl) st = run0[sm], b0 = spre[sm], b1 = sm + 1 < nsl ? spre[sm + 1] : total;
                const int nrun = min(64, (nsl - sb + NW - 1) / NW);
                for (int i = 0; i < nrun; ++i) {
                    const int B0 = read_lane(b0, i), x0 = max(B0, c0), x1 = min(read_lane(b1, i), c0 + cn);
                    if (x0 >= x1) continue;  // (wave-uniform)
                    const int rs0 = (sb + NW * i) << log_trg;
                    const int *src = went + (long long)rs0 * nt + read_lane(st, i) - B0;  // entry g of the concatenation, b0 <= g < b1
                    for (int g = x0 + lane; g < x1; g += 64) {
                        const int v = src[g], r = rs0 + ((v >> 12) & 31);
                        int ls = v & 0xfff;
                        if constexpr (ONES) {  // the replica's own spin bit at the site rides in bit 15 (these loads overlap across the workgroup)
                            int w32;
                            unsigned int bit;
                            rs_bit_of(tile0 + ls, w32, bit);
                            if (p.bits[(long long)r * p.nw32 + w32] & bit) ls |= 0x8000;
                        }
                        sent[g - c0] = (r << p.log_w) | (v >> 17);
                        sls[g - c0] = (unsigned short)ls;
                    }
                }
            }
        }
        __syncthreads();
        // the sorted chunk, a contiguous piece per quarter wave: the spin bits in registers up to NKMAX words of 16 bytes
        // per lane (one magnitude plane: n <= 16384), streamed per entry beyond
        const RsTileChunk ch{sent, sls, sjabs, prow, bits, p.base, cn, nw2, rw2, p.log_w, p.W, NW};
        // (the register budget of 1024 threads: 8 words per lane beside one magnitude plane, 4 beside three; eight
        //  magnitude planes -- nine LDS reads per word of spin bits -- always stream)
        constexpr int NKMAX = row_shared_tile_register_words(PL);
        const int nk = (nw2 + 15) >> 4;
        switch (nk <= NKMAX ? nk : 0) {
            case 1: rs_tile_pieces<PL, ONES, NKMAX >= 1 ? 1 : 0>(ch, wv, sub, l16); break;
            case 2: rs_tile_pieces<PL, ONES, NKMAX >= 2 ? 2 : 0>(ch, wv, sub, l16); break;
            case 3: rs_tile_pieces<PL, ONES, NKMAX >= 3 ? 3 : 0>(ch, wv, sub, l16); break;
            case 4: rs_tile_pieces<PL, ONES, NKMAX >= 4 ? 4 : 0>(ch, wv, sub, l16); break;
            case 5: rs_tile_pieces<PL, ONES, NKMAX >= 5 ? 5 : 0>(ch, wv, sub, l16); break;
            case 6: rs_tile_pieces<PL, ONES, NKMAX >= 6 ? 6 : 0>(ch, wv, sub, l16); break;
            case 7: rs_tile_pieces<PL, ONES, NKMAX >= 7 ? 7 : 0>(ch, wv, sub, l16); break;
            case 8: rs_tile_pieces<PL, ONES, NKMAX >= 8 ? 8 : 0>(ch, wv, sub, l16); break;
            default: rs_tile_pieces<PL, ONES, 0>(ch, wv, sub, l16); break;
        }
    }
}

// ---- fields by on-chip conversion (int8 rows with 8 magnitude planes): one workgroup (4 waves) per proposed site -------
// LDS: [PL + 1][4 nseg] 64-bit words (sign plane first).
template <typename JE, int PL, bool GRID>
__global__ void __launch_bounds__(256) rs_fields_kernel(const SweepArgs a, const RsPlanArg<GRID> pg, int win) {
    const RowSharedPlan &p = rs_plan(pg);
    const int i = blockIdx.x, n = a.n;
    const int *off = p.off + (long long)win * (n + 1);
    const int lo = off[i], hi = off[i + 1];
    if (lo == hi) return;  // nobody proposes this site in this window: the row is not read
    extern __shared__ unsigned long long planes[];
    __shared__ int csum[4];
    const int nseg = (n + 255) >> 8, nw = 4 * nseg;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const JE *row = reinterpret_cast<const JE *>(a.J) + (long long)i * a.ldj;
    int absum = rs_row_to_planes<JE, PL, GRID>(row, n, planes, lane, wv, rs_grid_k(pg));
    absum = wave_sum(absum);
    if (lane == 0) csum[wv] = absum;
    __syncthreads();
    const int C = csum[0] + csum[1] + csum[2] + csum[3];  // sum_j |J_ij|
    // sum_j J_ij s_j = C - 2 sum_b 2^b popcount(plane_b & (sign ^ spin bits))
    const unsigned long long *bits = reinterpret_cast<const unsigned long long *>(p.bits);
    const int wmask = (1 << p.log_w) - 1;
    for (int x = lo + wv; x < hi; x += 8) {  // two entries per wave at a time (wave-uniform bounds)
        const bool two = x + 4 < hi;
        const int e0 = p.ent[x], e1 = two ? p.ent[x + 4] : e0;
        const unsigned long long *s0 = bits + (long long)(e0 >> p.log_w) * nw;
        const unsigned long long *s1 = bits + (long long)(e1 >> p.log_w) * nw;
        int acc0 = 0, acc1 = 0;
        for (int c = lane; c < nw; c += 64) {
            const unsigned long long sg = planes[c];
            const unsigned long long x0 = s0[c] ^ sg, x1 = s1[c] ^ sg;
#pragma unroll
            for (int b = 0; b < PL; ++b) {
                const unsigned long long pb = planes[(long long)(1 + b) * nw + c];
                acc0 += __popcll(pb & x0) << b;
                acc1 += __popcll(pb & x1) << b;
            }
        }
        wave_sum2(acc0, acc1);
        if (lane == 0) {
            p.base[(long long)(e0 >> p.log_w) * p.W + (e0 & wmask)] = C - 2 * acc0;
            if (two) p.base[(long long)(e1 >> p.log_w) * p.W + (e1 & wmask)] = C - 2 * acc1;
        }
    }
}

// ---- chain: one wave per replica, W = 64 NB pending fields ---------------------------------------------------------
// The accept-table rule of the look-ahead form, evaluated per lane: ptab[q] = expf_det((float)(-(double)(2 q) / T)).
__device__ __forceinline__ bool rs_accept(float fk, float u, double T, int table_m) {
    if (fk <= 0.0f) return true;
    if (fk <= (float)table_m) return u < expf_det((float)(-(double)(2 * (int)fk) / T));
    const double dE = (double)(2.0f * fk);
    return (dE > T * 104.0) ? false : (u < expf_det((float)(-dE / T)));
}

// J[sa][site], sa wave-uniform, in two steps, so that several gathers are in flight before the first is looked at:
// rs_coupling_load issues the loads and rs_coupling decodes the float the row of J holds.  BITS: from the resident
// planes of row sa (one magnitude plane: two bits give nonzero ? (sign ? -1 : +1) : 0), (w32, bit) = rs_bit_of(site)
// -- a 40 KB fp32 row gathered at W sites costs about a cache line per lane, its plane row is 2.5 KB in all.
// ONES (with BITS): the problem is flagged sign-only -- every off-diagonal |J| is one unit -- so the magnitude word is
// known without a load: off the diagonal the coupling is +-unit by the sign bit, and on it (J_aa = 0) the two sites are
// the same, the very test the chain makes to negate a repeated site's spin.  Half the gathers per correction and candidate.
template <typename JE, bool BITS, bool ONES = false>
struct RsRaw {
    typename std::conditional<BITS, typename std::conditional<ONES, uint32_t, uint2>::type, JE>::type v;
};
// voff: the lane's byte offset in the row (BITS: of the 32-bit word of rs_bit_of(site) in a plane; else of J[.][site]),
// unsigned and 32 bits wide beside a wave-uniform row address
template <typename JE, bool BITS, bool ONES>
__device__ __forceinline__ void rs_coupling_load(RsRaw<JE, BITS, ONES> &raw, const SweepArgs &a, const RowSharedPlan &p, int sa,
                                                 unsigned int voff) {
    if constexpr (BITS && ONES) {
        const char *sgn = reinterpret_cast<const char *>(p.jp) + (long long)sa * (8ll * p.nw32);
        raw.v = *reinterpret_cast<const uint32_t *>(sgn + voff);
    } else if constexpr (BITS) {
        const char *sgn = reinterpret_cast<const char *>(p.jp) + (long long)sa * (8ll * p.nw32);
        const char *mag = sgn + 4ll * p.nw32;
        raw.v = make_uint2(*reinterpret_cast<const uint32_t *>(sgn + voff), *reinterpret_cast<const uint32_t *>(mag + voff));
    } else {
        const char *row = reinterpret_cast<const char *>(a.J) + (long long)sa * a.ldj * (long long)sizeof(JE);
        raw.v = *reinterpret_cast<const JE *>(row + voff);
    }
}
// unit: the value of one magnitude bit (1, GRID: 2^-k); rows of J itself are in real units already
template <typename JE, bool BITS>
__device__ __forceinline__ float rs_coupling(const RsRaw<JE, BITS> &raw, unsigned int bit, float unit) {
    if constexpr (BITS) return (raw.v.y & bit) ? ((raw.v.x & bit) ? -unit : unit) : 0.0f;
    else return (float)raw.v;
}
// ONES; same: the two sites are one -- the diagonal, whose coupling is 0
template <typename JE>
__device__ __forceinline__ float rs_coupling(const RsRaw<JE, true, true> &raw, unsigned int bit, float unit, bool same) {
    return same ? 0.0f : ((raw.v & bit) ? -unit : unit);
}

// Wave priority of the chain for its lifetime (s_setprio, 0 ... 3): beside another replica group's fields kernel a chain
// wave shares its SIMD with VALU-saturated waves, and its serial stretches -- a decision of 64 lanes, the selects of the
// current block -- wait for issue slots.  0: no instruction is emitted, the kernel is what it was.  The value is the
// measured one; -DSGA_RS_CHAIN_PRIO=0 builds the other side of the A/B.
#ifndef SGA_RS_CHAIN_PRIO
#define SGA_RS_CHAIN_PRIO 3
#endif
constexpr int RS_CHAIN_PRIO = SGA_RS_CHAIN_PRIO;
constexpr int RS_CHAIN_K = 4;  // candidates fetched per round (measured among 4, 8, 16)
constexpr int RS_CHAIN_U = 8;  // earlier accepts applied to a block per wait
// The accept probabilities of the integer Metropolis form from a table the wave fills once per window (DESIGN.md 7,
// "Chain: accept table"); -DSGA_RS_CHAIN_TABLE=0 builds the other side of the A/B, rs_accept per lane at every decision.
#ifndef SGA_RS_CHAIN_TABLE
#define SGA_RS_CHAIN_TABLE 1
#endif
constexpr bool RS_CHAIN_TABLE = SGA_RS_CHAIN_TABLE != 0;
// The prologue without a load under a lane condition ("Staged prologue"): the window's base slots are
// loaded raw for every lane (base is [R][W]), the gathers of h and spin follow their block's site, the accept table is
// filled, and the conversions of the base slots -- the first values that wait -- come last, so the compiler counts vmcnt
// down instead of draining it once per block.  -DSGA_RS_CHAIN_STAGED=0: base[tw] loaded and converted per block under
// the lane's condition, as it was.
#ifndef SGA_RS_CHAIN_STAGED
#define SGA_RS_CHAIN_STAGED 1
#endif
constexpr bool RS_CHAIN_STAGED = SGA_RS_CHAIN_STAGED != 0;
// The current block's values read from register vectors with the wave-uniform block index (NB = 16: indexed register
// moves; NB = 4, 8: the compiler's own select chain).  -DSGA_RS_CHAIN_INDEXED=0: arrays and one select over every block.
#ifndef SGA_RS_CHAIN_INDEXED
#define SGA_RS_CHAIN_INDEXED 1
#endif
constexpr bool RS_CHAIN_INDEXED = SGA_RS_CHAIN_INDEXED != 0;

// NB values of a lane, one per block of the window: written with constant indices
template <typename T, int NB>
struct RsBlockRegs {
#if SGA_RS_CHAIN_INDEXED
    typedef T V __attribute__((ext_vector_type(NB)));
    V v;
#else
    T v[NB];
#endif
};

// The decision of the integer Metropolis form from the wave's table (sga_kernels.h: rs_accept_table_entries, with the
// argument for "false beyond Q"): ptab[q] holds rs_accept's own expression for q = 1 ... Q, so u < ptab[q] is its
// decision bit for bit; zero_tail: Q == rs_accept_table_zero_from(T).  A q beyond a table that does not end in zeros is
// evaluated by rs_accept itself, in a branch the wave takes only when one of its lanes needs it.
__device__ __forceinline__ bool rs_accept_tabled(const float *ptab, int Q, bool zero_tail, float fk, float u, double T, int table_m) {
    if (fk <= 0.0f) return true;
    const int q = (int)fk;
    if (q <= Q) return u < ptab[q];
    if (zero_tail) return false;
    return rs_accept(fk, u, T, table_m);
}

// The blocks of the window (64 updates, one per lane) are walked in order.  A block is touched when it becomes
// current: first it takes the corrections of every accept made so far in the window -- field -= 2 J[i_a][site] s_a
// (J symmetric: read from row i_a), spin negated where the site repeats -- from the accept list in LDS, RS_CHAIN_U
// independent gathers per wait.  Then it is decided in rounds: the first RS_CHAIN_K accepting lanes are candidates,
// their couplings to the block are fetched together (a coupling depends on the two sites only, so it stays good
// whatever is committed meanwhile), and accepts are committed from registers for as long as the first accepting
// lane -- the chain's next accept: every lane before it rejects against fields that hold every earlier accept -- is
// the next candidate.  A candidate that stopped accepting is skipped; a lane that was not fetched and accepts first
// starts a new round.  One memory round trip per round, not per accept; the sums are integers below 2^24, so the
// order of the corrections does not matter.
// GRID: the fields are held in real units (2^-k times those integers: as exact, in any order), and the decision and
// dE are metropolis_accept's, the row kernels' general rule (the proof at the top of the file).
// ANYRULE: "accept" reads "flip" -- Glauber and heat bath by the same general rule, in either form of the fields.
template <bool GRID>
__device__ __forceinline__ bool rs_decide(int cs, float cf, float chh, float cu, double T, int table_m) {
    if constexpr (GRID) {
        double dE;
        return metropolis_accept(SGA_RULE_METROPOLIS, SGA_ARITH_F64, cf, cs, chh, 0.0f, T, cu, dE);
    } else {
        return rs_accept((float)cs * (cf + chh), cu, T, table_m);
    }
}
// ANYRULE: Glauber / heat bath (rule: a.rule, wave-uniform at run time) by the row kernels' general rule, in the integer
// form (cf the exact integer-valued field) and the GRID form alike; true: the spin flips.  Off: rs_decide, as it was.
template <bool GRID, bool ANYRULE>
__device__ __forceinline__ bool rs_decide_rule(int rule, int cs, float cf, float chh, float cu, double T, int table_m) {
    if constexpr (ANYRULE) {
        double dE;
        return metropolis_accept(rule, SGA_ARITH_F64, cf, cs, chh, 0.0f, T, cu, dE);
    } else {
        return rs_decide<GRID>(cs, cf, chh, cu, T, table_m);
    }
}

template <typename JE, int NB, bool BITS, bool GRID, bool ANYRULE = false, bool ONES = false>
__global__ void __launch_bounds__(64) rs_chain_kernel(const SweepArgs a, const RsPlanArg<GRID> pg, int k, int win) {
    const RowSharedPlan &p = rs_plan(pg);
    if constexpr (RS_CHAIN_PRIO > 0) __builtin_amdgcn_s_setprio(RS_CHAIN_PRIO);
    constexpr int W = 64 * NB, K = RS_CHAIN_K, U = RS_CHAIN_U;
    constexpr bool TABLE = RS_CHAIN_TABLE && !GRID && !ANYRULE;
    __shared__ uint32_t alist[W + U];  // the window's accepts in chain order: site | (spin before the flip < 0) << 31
    __shared__ float ptab[TABLE ? RS_ACCEPT_TABLE_MAX + 1 : 1];  // TABLE: the accept probabilities of this wave's T
    const int r = blockIdx.x, lane = threadIdx.x, n = a.n;
    const int t0 = win * W, cnt = min(W, n - t0);
    const double T = a.sched ? a.sched[k * a.sched_ss + r * a.sched_rs] : a.rep_temp[r];
    int8_t *srow = a.spins + (long long)r * a.sstride;
    const int *base = p.base + (long long)r * W;
    // the h of this replica's model (one matrix, many field vectors); resolved once, wave-uniform
    const float *hvec = a.h;
    if (a.reps_per_model > 0)
        hvec += (long long)__builtin_amdgcn_readfirstlane((int)((a.replica0 + (uint32_t)r) / (uint32_t)a.reps_per_model)) * n;
    const float unit = GRID ? ldexpf(1.0f, -rs_grid_k(pg)) : 1.0f;  // 2^-k
    RsBlockRegs<int, NB> site, s;
    RsBlockRegs<float, NB> f, hh, u;
    // the window's base slots, raw (base is [R][W]: a slot past cnt is in the array, its value unused)
    int braw[NB];
    if constexpr (RS_CHAIN_STAGED) {
#pragma unroll
        for (int b = 0; b < NB; ++b) braw[b] = base[64 * b + lane];
    }
    // sites, uniforms and the gathers of h and spin; a lane past cnt keeps site 0 and u 0
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int tw = 64 * b + lane;
        const bool valid = tw < cnt;
        uint32_t ub = 0;
        int sb = 0;
        if (valid) rs_update(a, r, k, t0 + tw, sb, ub);
        site.v[b] = sb;
        u.v[b] = (float)ub * 0x1.0p-24f;
        if constexpr (!RS_CHAIN_STAGED) {
            f.v[b] = valid ? (float)base[tw] : 0.0f;
            if constexpr (GRID) f.v[b] = ldexpf(f.v[b], -rs_grid_k(pg));  // 2^-k D, exact
        }
        hh.v[b] = hvec[sb];
        s.v[b] = srow[sb];
    }
    // The accept table of this wave's T, filled behind the loads above: rs_accept's expression for
    // q = 1 ... Q, Q / 64 entries per lane (entry 0 is never read: fk <= 0 accepts).
    int Q = 0;
    bool zero_tail = false;
    if constexpr (TABLE) {
        Q = __builtin_amdgcn_readfirstlane(rs_accept_table_entries(T, a.table_m));
        zero_tail = Q == __builtin_amdgcn_readfirstlane(rs_accept_table_zero_from(T));
        for (int q = lane; q <= Q; q += 64) ptab[q] = expf_det((float)(-(double)(2 * q) / T));
    }
    // the fields from the base slots -- the first values that wait
    if constexpr (RS_CHAIN_STAGED) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float fb = 64 * b + lane < cnt ? (float)braw[b] : 0.0f;
            if constexpr (GRID) fb = ldexpf(fb, -rs_grid_k(pg));  // 2^-k D, exact
            f.v[b] = fb;
        }
    }
    double E = a.energy[r];
    int nA = 0;  // accepts of this window so far
    const int nblk = (cnt + 63) >> 6;
    auto decide = [&](int cs, float cf, float chh, float cu) {
        if constexpr (TABLE) return rs_accept_tabled(ptab, Q, zero_tail, (float)cs * (cf + chh), cu, T, a.table_m);
        else return rs_decide_rule<GRID, ANYRULE>(a.rule, cs, cf, chh, cu, T, a.table_m);
    };
    for (int cb = 0; cb < nblk; ++cb) {
        int csite = 0, cs = 0;
        float cf = 0.0f, chh = 0.0f, cu = 0.0f;
        if constexpr (RS_CHAIN_INDEXED) {
            csite = site.v[cb], cs = s.v[cb], cf = f.v[cb], chh = hh.v[cb], cu = u.v[cb];
        } else {
#pragma unroll
            for (int b = 0; b < NB; ++b)
                if (b == cb) csite = site.v[b], cs = s.v[b], cf = f.v[b], chh = hh.v[b], cu = u.v[b];
        }
        const bool cvalid = 64 * cb + lane < cnt;
        unsigned int voff = (unsigned int)csite * (unsigned int)sizeof(JE), bit = 0;
        if constexpr (BITS) {
            int w32;
            rs_bit_of(csite, w32, bit);
            voff = 4u * (unsigned int)w32;
        }
        // The fence of the accept list: the workgroup is one wave, so no barrier is executed, but neither the compiler
        // nor the LDS queue may move the reads below ahead of lane 0's stores to alist (wave-uniform control flow).
        __syncthreads();
        for (int k0 = 0; k0 < nA; k0 += U) {
            uint32_t e[U];
            RsRaw<JE, BITS, ONES> x[U];
#pragma unroll
            for (int j = 0; j < U; ++j) e[j] = alist[k0 + j];  // (past nA: in the array, unused)
#pragma unroll
            for (int j = 0; j < U; ++j) {
                x[j] = RsRaw<JE, BITS, ONES>{};
                if (k0 + j < nA) {  // wave-uniform, here and below
                    e[j] = (uint32_t)__builtin_amdgcn_readfirstlane((int)e[j]);
                    rs_coupling_load<JE, BITS, ONES>(x[j], a, p, (int)(e[j] & 0x7fffffffu), voff);
                }
            }
#pragma unroll
            for (int j = 0; j < U; ++j) {
                if (k0 + j < nA) {
                    if constexpr (ONES) {
                        const bool same = csite == (int)(e[j] & 0x7fffffffu);
                        cf -= rs_coupling<JE>(x[j], bit, unit, same) * ((e[j] >> 31) ? -2.0f : 2.0f);
                        if (same) cs = -cs;
                    } else {
                        cf -= rs_coupling<JE, BITS>(x[j], bit, unit) * ((e[j] >> 31) ? -2.0f : 2.0f);
                        if (csite == (int)(e[j] & 0x7fffffffu)) cs = -cs;
                    }
                }
            }
        }
        bool acc = cvalid && decide(cs, cf, chh, cu);
        unsigned long long m = ballot64(acc);  // accepting lanes among the undecided ones
        while (m) {
            int cl[K];
            RsRaw<JE, BITS, ONES> x[K];
            unsigned long long rest = m;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                cl[j] = rest ? (int)__builtin_ctzll(rest) : 64;
                rest &= rest - 1;
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                x[j] = RsRaw<JE, BITS, ONES>{};
                if (cl[j] < 64) rs_coupling_load<JE, BITS, ONES>(x[j], a, p, read_lane(csite, cl[j]), voff);  // wave-uniform
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (!m) break;
                const int fl = (int)__builtin_ctzll(m);
                if (fl < cl[j]) break;      // not fetched (or the candidates are used up): the next round
                if (fl > cl[j]) continue;   // candidate j accepts no longer
                const int sa = read_lane(csite, fl), ss = read_lane(cs, fl);
                if constexpr (GRID || ANYRULE) {  // metropolis_accept's dE, formed as it forms it
                    E += 2.0 * (double)ss * ((double)read_lane(cf, fl) + (double)read_lane(chh, fl));
                } else {
                    const float fk = (float)ss * (read_lane(cf, fl) + read_lane(chh, fl));
                    E += (double)(2.0f * fk);
                }
                if (lane == 0) {
                    srow[sa] = (int8_t)(-ss);
                    int aw;
                    unsigned int ab;
                    rs_bit_of(sa, aw, ab);
                    atomicXor(&p.bits[(long long)r * p.nw32 + aw], ab);
                    alist[nA] = (uint32_t)sa | (ss < 0 ? 0x80000000u : 0u);
                }
                ++nA;
                if constexpr (ONES) cf -= rs_coupling<JE>(x[j], bit, unit, csite == sa) * (2.0f * (float)ss);
                else cf -= rs_coupling<JE, BITS>(x[j], bit, unit) * (2.0f * (float)ss);
                if (csite == sa) cs = -cs;
                acc = cvalid && decide(cs, cf, chh, cu);
                m = ballot64(acc) & (~1ull << fl);
            }
        }
    }
    if (lane == 0) {
        a.energy[r] = E;
        a.n_accepted[r] += (unsigned long long)nA;
        if (t0 + cnt == n && a.energy_trace) a.energy_trace[(long long)k * a.R + r] = E;
    }
}

template <typename Kern, typename Plan>
static hipError_t rs_launch_fields(Kern kern, size_t lds, const SweepArgs &a, const Plan &p, int win, hipStream_t st) {
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(a.n), dim3(256), lds, st, a, p, win);
    return hipGetLastError();
}

// the tile kernel's instantiation for (planes, ones); null: none
static const void *rs_tiles_kernel_of(int planes, bool ones) {
    if (ones) return planes == 1 ? reinterpret_cast<const void *>(rs_fields_tiles_kernel<1, true>) : nullptr;
    switch (planes) {
        case 1: return reinterpret_cast<const void *>(rs_fields_tiles_kernel<1, false>);
        case 3: return reinterpret_cast<const void *>(rs_fields_tiles_kernel<3, false>);
        case 8: return reinterpret_cast<const void *>(rs_fields_tiles_kernel<8, false>);
        default: return nullptr;
    }
}
hipError_t row_shared_tiles_prepare(int planes, bool ones, size_t lds_bytes) {
    const void *kern = rs_tiles_kernel_of(planes, ones);
    if (!kern || lds_bytes > RS_TILE_LDS_BUDGET) return hipErrorInvalidValue;
    return ensure_lds_limit(kern, lds_bytes);
}
template <typename Kern>
static hipError_t rs_launch_tiles(Kern kern, const SweepArgs &a, const RowSharedPlan &p, const RowSharedTiles &t, int log_trg,
                                  int win, hipStream_t st) {
    const size_t lds = row_shared_tile_lds(a.n, p.planes, t.ones != 0, t.S, a.R);
    hipError_t e = ensure_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((a.n + t.S - 1) / t.S), dim3(RS_TILE_THREADS), lds, st, a, p, t.S, log_trg, win);
    return hipGetLastError();
}
static hipError_t rs_fields_tiles(const SweepArgs &a, const RowSharedPlan &p, const RowSharedTiles &t, int log_trg, int win,
                                  hipStream_t st) {
    if (t.ones) return rs_launch_tiles(rs_fields_tiles_kernel<1, true>, a, p, t, log_trg, win, st);
    switch (p.planes) {
        case 1: return rs_launch_tiles(rs_fields_tiles_kernel<1, false>, a, p, t, log_trg, win, st);
        case 3: return rs_launch_tiles(rs_fields_tiles_kernel<3, false>, a, p, t, log_trg, win, st);
        case 8: return rs_launch_tiles(rs_fields_tiles_kernel<8, false>, a, p, t, log_trg, win, st);
        default: return hipErrorInvalidValue;
    }
}

template <typename JE>
static hipError_t rs_fields(const SweepArgs &a, const RowSharedPlan &p, int grid, const RowSharedTiles &tiles, int log_trg, int win,
                            hipStream_t st) {
    const size_t lds = (size_t)(p.planes + 1) * (p.nw32 / 2) * 8;
    if (p.jp && tiles.S > 0) return rs_fields_tiles(a, p, tiles, log_trg, win, st);
    if (p.jp) {
        switch (p.planes) {
            case 1: return rs_launch_fields(rs_fields_planes_kernel<1>, lds, a, p, win, st);
            case 3: return rs_launch_fields(rs_fields_planes_kernel<3>, lds, a, p, win, st);
            case 8: return rs_launch_fields(rs_fields_planes_kernel<8>, lds, a, p, win, st);
            default: return hipErrorInvalidValue;
        }
    }
    if constexpr (std::is_same<JE, float>::value) {  // (int8 rows are integers: k = 0, the planes are the integer form's)
        if (grid > 1) {
            const RowSharedGridPlan g{p, grid - 1};
            switch (p.planes) {
                case 1: return rs_launch_fields(rs_fields_kernel<JE, 1, true>, lds, a, g, win, st);
                case 3: return rs_launch_fields(rs_fields_kernel<JE, 3, true>, lds, a, g, win, st);
                case 8: return rs_launch_fields(rs_fields_kernel<JE, 8, true>, lds, a, g, win, st);
                default: return hipErrorInvalidValue;
            }
        }
    }
    switch (p.planes) {
        case 1: return rs_launch_fields(rs_fields_kernel<JE, 1, false>, lds, a, p, win, st);
        case 3: return rs_launch_fields(rs_fields_kernel<JE, 3, false>, lds, a, p, win, st);
        case 8: return rs_launch_fields(rs_fields_kernel<JE, 8, false>, lds, a, p, win, st);
        default: return hipErrorInvalidValue;
    }
}

template <typename JE, bool BITS, bool GRID, bool ANYRULE, bool ONES>
static hipError_t rs_chain_launch(const SweepArgs &a, const RsPlanArg<GRID> &p, int W, int k, int win, hipStream_t st) {
    switch (W) {
        case 256: hipLaunchKernelGGL((rs_chain_kernel<JE, 4, BITS, GRID, ANYRULE, ONES>), dim3(a.R), dim3(64), 0, st, a, p, k, win); break;
        case 512: hipLaunchKernelGGL((rs_chain_kernel<JE, 8, BITS, GRID, ANYRULE, ONES>), dim3(a.R), dim3(64), 0, st, a, p, k, win); break;
        case 1024: hipLaunchKernelGGL((rs_chain_kernel<JE, 16, BITS, GRID, ANYRULE, ONES>), dim3(a.R), dim3(64), 0, st, a, p, k, win); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
// (Glauber / heat bath: the ANYRULE instantiations; the rule itself stays a run-time value in them)
// ONES: the rows are sign-only (RowSharedTiles::ones, known where the tile kernel runs): the BITS chain gathers sign words alone
template <typename JE, bool BITS, bool ONES = false>
static hipError_t rs_chain(const SweepArgs &a, const RowSharedPlan &p, int grid, int k, int win, hipStream_t st) {
    if (a.rule != SGA_RULE_METROPOLIS) {
        if (grid) return rs_chain_launch<JE, BITS, true, true, ONES>(a, RowSharedGridPlan{p, grid - 1}, p.W, k, win, st);
        return rs_chain_launch<JE, BITS, false, true, ONES>(a, p, p.W, k, win, st);
    }
    if (grid) return rs_chain_launch<JE, BITS, true, false, ONES>(a, RowSharedGridPlan{p, grid - 1}, p.W, k, win, st);
    return rs_chain_launch<JE, BITS, false, false, ONES>(a, p, p.W, k, win, st);
}

template <typename JE>
static hipError_t rs_build_planes(const void *J, long long ldj, int n, int planes, unsigned long long *jp, int *jabs,
                                  hipStream_t st) {
    const JE *Jt = reinterpret_cast<const JE *>(J);
    switch (planes) {
        case 1: hipLaunchKernelGGL((rs_planes_kernel<JE, 1>), dim3(n), dim3(256), 0, st, Jt, ldj, n, jp, jabs); break;
        case 3: hipLaunchKernelGGL((rs_planes_kernel<JE, 3>), dim3(n), dim3(256), 0, st, Jt, ldj, n, jp, jabs); break;
        case 8: hipLaunchKernelGGL((rs_planes_kernel<JE, 8>), dim3(n), dim3(256), 0, st, Jt, ldj, n, jp, jabs); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
static hipError_t rs_build_planes_grid(const void *J, long long ldj, int n, int planes, int gk, unsigned long long *jp, int *jabs,
                                       hipStream_t st) {
    const float *Jt = reinterpret_cast<const float *>(J);
    switch (planes) {
        case 1: hipLaunchKernelGGL((rs_planes_grid_kernel<1>), dim3(n), dim3(256), 0, st, Jt, ldj, n, jp, jabs, gk); break;
        case 3: hipLaunchKernelGGL((rs_planes_grid_kernel<3>), dim3(n), dim3(256), 0, st, Jt, ldj, n, jp, jabs, gk); break;
        case 8: hipLaunchKernelGGL((rs_planes_grid_kernel<8>), dim3(n), dim3(256), 0, st, Jt, ldj, n, jp, jabs, gk); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_rs_build_planes(const void *J, bool j_is_i8, long long ldj, int n, int planes, int grid_k,
                                  unsigned long long *jp, int *jabs, hipStream_t st) {
    if (!J || !jp || !jabs || n <= 0 || grid_k < 0 || grid_k > 30 || (j_is_i8 && grid_k != 0)) return hipErrorInvalidValue;
    if (j_is_i8) return rs_build_planes<int8_t>(J, ldj, n, planes, jp, jabs, st);
    return grid_k ? rs_build_planes_grid(J, ldj, n, planes, grid_k, jp, jabs, st)
                  : rs_build_planes<float>(J, ldj, n, planes, jp, jabs, st);
}

// One replica group of a launch: the group's own arguments and plan view (a one-group launch: the call's), its stream and
// the geometry of its plan launches.
struct RsGroupLaunch {
    SweepArgs a;
    RowSharedPlan p;
    hipStream_t st = nullptr;
    RowSharedTilePlan tp;
    size_t tlds = 0;
    int log_trg = 0;
    dim3 pgrid, tgrid;
};

// replicas [r0, r1) of the call as an engine of their own: every per-replica pointer advanced, the plan's scratch carved
// (row_shared_group_view); Philox streams and the model of a shared-coupling batch go through replica0 + r
static void rs_group_args(const SweepArgs &a, const RowSharedPlan &p, const RowSharedGroups &g, int i, SweepArgs &ag, RowSharedPlan &pg) {
    const int r0 = g.begin[i];
    const RowSharedGroupView v = row_shared_group_view(a.n, p.W, g, i);
    ag = a;
    ag.R = g.begin[i + 1] - r0;
    ag.replica0 = a.replica0 + (uint32_t)r0;
    ag.spins = a.spins + (long long)r0 * a.sstride;
    ag.energy = a.energy + r0;
    ag.best_energy = a.best_energy ? a.best_energy + r0 : nullptr;
    ag.best_spins = a.best_spins ? a.best_spins + (long long)r0 * a.sstride : nullptr;
    ag.n_accepted = a.n_accepted + r0;
    ag.rep_temp = a.rep_temp ? a.rep_temp + r0 : nullptr;
    ag.sched = a.sched ? a.sched + (long long)r0 * a.sched_rs : nullptr;
    pg = p;
    pg.cnt = p.cnt + v.cnt;
    pg.ent = p.ent + v.ent;
    pg.base = p.base + v.base;
    pg.bits = p.bits + v.bits;
    pg.n_groups = v.n_groups;
}

hipError_t launch_sweep_dense_rs(const SweepArgs &a, const RowSharedPlan &p, bool j_is_i8, hipStream_t st, int grid,
                                 RowSharedTiles tiles, const RowSharedGroupRun *run) {
    // the tile kernel: resident planes, the image and the replica counters within LDS (the host rule saw to it), sign-only
    // rows only where the planes are one magnitude plane
    if (tiles.S > 0 && (!p.jp || tiles.S > RS_TILE_MAX_SITES || a.R > RS_TILE_MAX_REPLICAS || (tiles.ones && p.planes != 1) ||
                        row_shared_tile_lds(a.n, p.planes, tiles.ones != 0, tiles.S, a.R) > RS_TILE_LDS_BUDGET))
        return hipErrorInvalidValue;
    // (its entry loop's 32-bit byte offsets: a group's spin bits within 2^30 bytes, a replica's within 2^18; base is 4 R W <= 2^24)
    if (tiles.S > 0 && (4ll * p.nw32 >= (1ll << 18) || 4ll * p.nw32 * a.R > (1ll << 30))) return hipErrorInvalidValue;
    // (many models: only over one shared matrix -- the plan buckets proposals by site, whatever the replica's model)
    if (a.reps_per_model < 0 || (a.reps_per_model > 0 && a.model_stride_j != 0)) return hipErrorInvalidValue;
    if (a.rep_list || a.R <= 0 || a.n <= 0 || (p.W != 256 && p.W != 512 && p.W != 1024) || (1 << p.log_w) != p.W)
        return hipErrorInvalidValue;
    if (p.log_rg < 0 || p.n_groups != (a.R + (1 << p.log_rg) - 1) >> p.log_rg || (p.jp && !p.jabs) || !p.tot)
        return hipErrorInvalidValue;
    if (grid < 0 || grid > 31 || (j_is_i8 && grid > 1)) return hipErrorInvalidValue;  // (int8 rows: k = 0)
    // the single-site rules; Glauber and heat bath decide in fp64 only (sga_sweep refuses them fp32 arithmetic)
    if (a.rule != SGA_RULE_METROPOLIS && a.rule != SGA_RULE_GLAUBER && a.rule != SGA_RULE_HEAT_BATH) return hipErrorInvalidValue;
    if (a.rule != SGA_RULE_METROPOLIS && a.arith != SGA_ARITH_F64) return hipErrorInvalidValue;
    const int nwin = (a.n + p.W - 1) / p.W;
    const size_t plds = sizeof(int) * (size_t)(a.n < RS_PLAN_TILE ? a.n : RS_PLAN_TILE);
    const dim3 sgrid(row_shared_scan_chunks(a.n), nwin);
    const bool chain_bits = p.jp && p.planes == 1;
    // the tile kernel takes its entries by (slice, tile, replica): one launch of the plan (row_shared_tile_plan)
    const bool by_tile = p.jp && tiles.S > 0;
    const bool chain_ones = chain_bits && by_tile && tiles.ones;  // sign-only rows (the flag travels with the tiles): sign words alone
    const int ntiles = by_tile ? (a.n + tiles.S - 1) / tiles.S : 0;
    // Replica groups: only over the tile plan (the by-site plan orders its entries across all replicas), only without an
    // energy trace (its stride is the call's R), and only in a geometry the pure rule admits; the caller asked the same rule.
    const RowSharedGroups groups = row_shared_groups(a.R, run ? run->G : 1);
    const int G = groups.G;
    if (run && run->G > 1 && (G != run->G || !by_tile || a.energy_trace || !run->fork || !row_shared_groups_fit(a.n, p.W, tiles.S, a.R, groups)))
        return hipErrorInvalidValue;
    RsGroupLaunch gl[RS_MAX_GROUPS];
    for (int g = 0; g < G; ++g) {
        RsGroupLaunch &q = gl[g];
        if (G > 1) {
            rs_group_args(a, p, groups, g, q.a, q.p);
            q.st = g ? run->stream[g - 1] : st;
            if (g && (!q.st || !run->join[g - 1])) return hipErrorInvalidValue;
        } else {
            q.a = a, q.p = p, q.st = st;
        }
        q.pgrid = dim3(q.p.n_groups, nwin, (a.n + RS_PLAN_TILE - 1) / RS_PLAN_TILE);
        if (by_tile) {
            q.tp = row_shared_tile_plan(a.n, p.W, tiles.S, q.a.R);
            if (q.tp.rg <= 0) return hipErrorInvalidValue;
            while ((1 << q.log_trg) < q.tp.rg) ++q.log_trg;
            q.tlds = row_shared_tile_plan_lds(p.W, q.tp.rg, q.tp.tiles);
            const hipError_t le = ensure_lds_limit(reinterpret_cast<const void *>(rs_tile_plan_kernel), q.tlds);
            if (le != hipSuccess) return le;
        }
        q.tgrid = dim3(by_tile ? (q.a.R + q.tp.rg - 1) / q.tp.rg : 1, nwin, by_tile ? (ntiles + q.tp.tiles - 1) / q.tp.tiles : 1);
    }
    hipError_t e = hipSuccess;
    if (G > 1) {  // fork: every group's stream behind what the call's stream holds
        e = hipEventRecord(run->fork, st);
        for (int g = 1; g < G && e == hipSuccess; ++g) e = hipStreamWaitEvent(gl[g].st, run->fork, 0);
        if (e != hipSuccess) return e;
    }
    // The groups' launches are issued turn by turn -- every group's plan, then window by window every group's fields and
    // chain -- so that no stream runs dry while the host fills another; inside a stream the order is the one-group order,
    // and nothing orders two groups against each other before the join: a group runs ahead across sweep boundaries.
    for (int g = 0; g < G && e == hipSuccess; ++g) {
        hipLaunchKernelGGL(rs_pack_kernel, dim3(gl[g].a.R), dim3(256), 0, gl[g].st, gl[g].a, gl[g].p);
        e = hipGetLastError();
    }
    for (int k = 0; k < a.n_sweeps && e == hipSuccess; ++k) {
        for (int g = 0; g < G && e == hipSuccess; ++g) {
            const RsGroupLaunch &q = gl[g];
            if (by_tile) {
                hipLaunchKernelGGL(rs_tile_plan_kernel, q.tgrid, dim3(RS_TILE_PLAN_THREADS), q.tlds, q.st, q.a, q.p, k, tiles.S, q.log_trg,
                                   q.tp.tiles);
            } else {
                hipLaunchKernelGGL(rs_plan_kernel<false>, q.pgrid, dim3(256), plds, q.st, q.a, q.p, k);
                hipLaunchKernelGGL(rs_scan_totals_kernel, sgrid, dim3(RS_SCAN_CHUNK), 0, q.st, q.a, q.p);
                hipLaunchKernelGGL(rs_scan_kernel, sgrid, dim3(RS_SCAN_CHUNK), 0, q.st, q.a, q.p);
                hipLaunchKernelGGL(rs_plan_kernel<true>, q.pgrid, dim3(256), plds, q.st, q.a, q.p, k);
            }
            e = hipGetLastError();
        }
        for (int w = 0; w < nwin && e == hipSuccess; ++w) {
            for (int g = 0; g < G && e == hipSuccess; ++g) {
                const RsGroupLaunch &q = gl[g];
                e = j_is_i8 ? rs_fields<int8_t>(q.a, q.p, grid, tiles, q.log_trg, w, q.st)
                            : rs_fields<float>(q.a, q.p, grid, tiles, q.log_trg, w, q.st);
                if (e != hipSuccess) break;
                if (chain_ones)
                    e = j_is_i8 ? rs_chain<int8_t, true, true>(q.a, q.p, grid, k, w, q.st) : rs_chain<float, true, true>(q.a, q.p, grid, k, w, q.st);
                else if (chain_bits)
                    e = j_is_i8 ? rs_chain<int8_t, true>(q.a, q.p, grid, k, w, q.st) : rs_chain<float, true>(q.a, q.p, grid, k, w, q.st);
                else
                    e = j_is_i8 ? rs_chain<int8_t, false>(q.a, q.p, grid, k, w, q.st) : rs_chain<float, false>(q.a, q.p, grid, k, w, q.st);
            }
        }
        // sweep boundary: best tracking (annealing/gpu_annealer.py:151-153), the energy is in a.energy
        for (int g = 0; g < G && e == hipSuccess && !a.no_best; ++g) {
            const RsGroupLaunch &q = gl[g];
            e = launch_update_best(q.a.energy, q.a.spins, q.a.best_energy, q.a.best_spins, q.a.sstride, q.a.R, q.st);
        }
    }
    if (G > 1) {  // join, whatever happened in between: nothing else uses the call's stream before every group is done
        hipError_t je = hipSuccess;
        for (int g = 1; g < G; ++g) {
            hipError_t x = hipEventRecord(run->join[g - 1], gl[g].st);
            if (x == hipSuccess) x = hipStreamWaitEvent(st, run->join[g - 1], 0);
            if (x != hipSuccess) (void)hipStreamSynchronize(gl[g].st), je = x;
        }
        if (e == hipSuccess) e = je;
    }
    if (e == hipSuccess) {
        // (the words "fields from resident bit-planes" / "on-chip conversion" are read by tests and bench.py)
        char gs[48] = "", ts[64] = "", rg[24] = "";
        if (grid) std::snprintf(gs, sizeof(gs), ", grid=2^-%d", grid - 1);
        if (a.rule != SGA_RULE_METROPOLIS)  // (Metropolis strings stay as they were)
            std::snprintf(gs + std::strlen(gs), sizeof(gs) - std::strlen(gs), ", rule=%s", a.rule == SGA_RULE_GLAUBER ? "glauber" : "heat-bath");
        if (p.jp && tiles.S > 0) std::snprintf(ts, sizeof(ts), " in tiles of %d sites%s", tiles.S, tiles.ones ? ", sign-only" : "");
        if (G > 1) std::snprintf(rg, sizeof(rg), " groups=%d", G);  // (one group: the string stays as it was)
        note_sweep_kernel("sweep_dense_rs<%s, planes=%d, W=%d%s> (row-shared windows: plan, fields from %s%s, chain)%s",
                          j_is_i8 ? "int8_t" : "float", p.planes, p.W, gs, p.jp ? "resident bit-planes" : "on-chip conversion", ts, rg);
    }
    return e;
}

}  // namespace sga
