// sga_replicas.h -- measurements and moves over the replicas beside the sweeps: observables.hip, cluster_moves.hip,
// resample.hip, pair_overlaps.hip and class_overlaps.hip.  The pure half: plans, argument records, the checks of the
// callers' lists and the launch declarations -- no sga_engine and no HIP call, so the plan programs under tests/c_abi pin
// it on the CPU.  The engine half is sga_replicas.cpp.
#ifndef SGA_REPLICAS_H
#define SGA_REPLICAS_H
#include <cstdio>
#include "sga_kernels.h"

namespace sga {

// The preamble of the three calls that pair ladder 2c with ladder 2c + 1 slot by slot (sga_cluster_move_ladders,
// sga_accumulate_ladder_overlaps, sga_accumulate_ladder_class_overlaps): why == nullptr where the slot range is served,
// and then L, the slots of a ladder.  noun: what the call pairs them for ("cluster moves" | "overlaps").  The text stands
// in a buffer of the calling thread until that thread asks again.
struct LadderPairs {
    const char *why;
    int L;
};
inline LadderPairs ladder_pairs_check(int n_ladders, bool have_slot_map, int R, int Rg, int slot_lo, int slot_hi, const char *noun) {
    static thread_local char text[160];
    if (n_ladders <= 0 || !have_slot_map) return {"no ladder (call sga_set_ladder)", 0};
    const char *need = n_ladders % 2 != 0 ? "an even number of ladders" : R != Rg ? "every replica on this rank (R_local == R_global)" : nullptr;
    if (need) {
        std::snprintf(text, sizeof(text), "%s between ladders need %s", noun, need);
        return {text, 0};
    }
    const int L = Rg / n_ladders;
    return {slot_lo < 0 || slot_hi > L || slot_lo > slot_hi ? "slot range outside [0, slots)" : nullptr, L};
}

// Replica observables (observables.hip; sga_get_magnetizations / sga_get_overlaps / sga_get_overlaps_with): the exact
// integer product Q = A B^T of two sets of row-major int8 rows over sites 0 ... n - 1, on the int8 matrix cores.  A
// workgroup takes one tile of OBS_TILE rows of A x OBS_TILE rows of B over one K range; the ranges' partial sums meet
// in int32 atomics (exact in any order).  The geometry is a pure function of (n, rows_a, rows_b, cus): no device call.
constexpr int OBS_TILE = 128;    // rows of A, and of B, per workgroup (2 x 2 waves of 64 x 64, as sweep_dense_seq.hip)
constexpr int OBS_K_GRAIN = 128; // a K range is a multiple of this (four K steps of 32 columns, loaded together)
constexpr int OBS_K_MIN = 512;   // no K range shorter than this: below it a split buys less than its atomics cost
struct ObservablesPlan {
    int tiles_m = 0, tiles_n = 0;  // tiles over the rows of A and of B
    int ksplit = 0;                // K ranges (1: plain stores, no zeroing of the result)
    int kchunk = 0;                // columns per K range; range s is [s kchunk, min(n, (s + 1) kchunk))
};
// The rule: about two workgroups per compute unit, as far as ranges of at least OBS_K_MIN columns allow.
inline ObservablesPlan observables_plan(int n, int rows_a, int rows_b, int cus) {
    ObservablesPlan p;
    if (n <= 0 || rows_a <= 0 || rows_b <= 0) return p;
    p.tiles_m = (rows_a + OBS_TILE - 1) / OBS_TILE;
    p.tiles_n = (rows_b + OBS_TILE - 1) / OBS_TILE;
    const long long tiles = (long long)p.tiles_m * p.tiles_n;
    const long long want = (2ll * (cus > 0 ? cus : 1) + tiles - 1) / tiles;
    const long long most = ((long long)n + OBS_K_MIN - 1) / OBS_K_MIN;
    const long long s = want < most ? want : most;  // (>= 1)
    const long long per = ((long long)n + s - 1) / s;
    p.kchunk = (int)((per + OBS_K_GRAIN - 1) / OBS_K_GRAIN * OBS_K_GRAIN);
    p.ksplit = (int)(((long long)n + p.kchunk - 1) / p.kchunk);
    return p;
}
struct ObservablesArgs {
    const int8_t *A;  // [rows_a][lda]
    const int8_t *B;  // [rows_b][ldb]
    int *out;         // out[a * ldq + b]; zeroed by the caller where plan.ksplit > 1
    long long lda, ldb, ldq;
    int rows_a, rows_b, n;
    int symmetric;    // A and B are the same rows: only the tiles with a <= b are computed, both halves written
    ObservablesPlan plan;
};
// Rows whose base and stride are multiples of 16 bytes are read 16 bytes per lane; any other operand byte by byte.
// Columns k >= n never enter the sums, whatever the rows hold there.
hipError_t launch_observables_product(const ObservablesArgs &a, hipStream_t st);
// out[r] = sum_{i < n} S[r][i]: one workgroup per row
hipError_t launch_observables_row_sums(const int8_t *S, long long ld, int n, int R, int *out, hipStream_t st);

// Isoenergetic cluster moves between two replicas of one sparse Hamiltonian (cluster_moves.hip; sga_cluster_move_pairs /
// sga_cluster_move_ladders; Houdayer 2001, Zhu, Ochoa and Katzgraber 2015): one workgroup of 256 threads per pair.  The
// sites where the two replicas differ, the cluster, and the two frontiers of a level-synchronous breadth-first search
// are bitmaps of ceil(n / 32) words in LDS; the connected component of differing sites around one drawn site is flipped
// in both replicas.  Rows are walked from rowptr64[i] to rowptr64[i + 1] of cv; an entry whose value is +-0 (padding,
// a stored zero) connects nothing.
constexpr int CLUSTER_THREADS = 256;
constexpr size_t CLUSTER_LDS_BUDGET = 160 * 1024 - 256;  // what the other kernels allow themselves
constexpr size_t CLUSTER_LDS_FIXED = 64;                 // wave sums and prefixes, the level's flag
inline size_t cluster_lds_bytes(long long n) { return 16 * (size_t)((n + 31) / 32) + CLUSTER_LDS_FIXED; }
// the largest n the bitmaps hold: 327 040 sites
constexpr long long CLUSTER_MAX_N = (long long)((CLUSTER_LDS_BUDGET - CLUSTER_LDS_FIXED) / 16) * 32;
// The pair list of sga_cluster_move_pairs, checked on the host before anything is enqueued: nullptr, or what is wrong
// with it.  reps_per_model > 0 (sga_set_csr_shared): both replicas of a pair under one field vector.  seen: R bytes.
inline const char *cluster_pairs_check(const int32_t *pairs, int count, int R, int replica0, int reps_per_model,
                                       unsigned char *seen) {
    for (int r = 0; r < R; ++r) seen[r] = 0;
    for (int k = 0; k < count; ++k) {
        const int a = pairs[2 * k], b = pairs[2 * k + 1];
        if (a < 0 || a >= R || b < 0 || b >= R) return "replica index out of range";
        if (a == b) return "a pair names one replica twice (a == b)";
        if (seen[a] || seen[b]) return "a replica is named in more than one pair";
        seen[a] = seen[b] = 1;
        if (reps_per_model > 0 && (replica0 + a) / reps_per_model != (replica0 + b) / reps_per_model)
            return "shared-coupling CSR batch: a pair joins replicas of two models (their field vectors differ)";
    }
    return nullptr;
}
struct ClusterArgs {
    int8_t *spins;                   // [R][sstride], sstride a multiple of 16
    const long long *rowptr64;       // [n + 1]
    const int2 *cv;                  // (column, value bits)
    unsigned long long *n_accepted;  // [R]: both replicas' counters grow by the cluster's size
    const int32_t *pairs;            // pair form: [count][2] local replicas
    const int32_t *slot_to_rep;      // ladder form (pairs == null): the slot map, [n_ladders][L] global ids
    int L, slot_lo, n_slots;         // ... pair p: ladders 2 (p / n_slots) and 2 (p / n_slots) + 1, slot slot_lo + p % n_slots
    int *sizes;                      // [count] cluster sizes, or null
    int *touched;                    // [R], zeroed by the caller: 1 where a replica's spins changed
    int n, sstride, R, count;
    uint32_t replica0, seed_lo, seed_hi, round;
};
hipError_t launch_cluster_moves(const ClusterArgs &a, hipStream_t st);
// After the energies were formed again: an untouched replica gets its saved energy back; a touched one's best follows
// where the new energy is lower (launch_update_best's step).
hipError_t launch_cluster_finish(const int *touched, const double *saved_energy, double *energy, const int8_t *spins,
                                 double *best_energy, int8_t *best_spins, int sstride, int R, hipStream_t st);

// Population annealing's resampling step (resample.hip; sga_resample; Hukushima and Iba 2003, Machta 2010): the local
// replicas in n_pop contiguous populations of N members, each copied or culled in proportion to exp(-dbeta E), exact in
// integers.  For population p with members r = 0 ... N - 1:
//   x_r = (-dbeta[p]) * E_r (one fp64 product), x_max = max_r x_r, W_r = (uint64)(exp_det(x_r - x_max) * 2^40) (the product
//   exact, the cast truncating; exp_det(0) == 1, so S = sum W_r >= 2^40; N <= 2^23 keeps S < 2^64), C_r = W_0 + ... + W_r;
//   one draw U of 64 bits (sweep_common.h, resample_draw), the offset o = (U * S) >> 64 < S;
//   child k = 0 ... N - 1 sits at t_k = k S + o, its parent is the r with N C_{r-1} <= t_k < N C_r (128-bit compares), so
//   n_r, the children of r, is the floor or the ceiling of N W_r / S and sum n_r = N;
//   every r with n_r >= 1 keeps its slot; the slots with n_r == 0, ascending, receive the surplus list -- parent r repeated
//   n_r - 1 times, ascending in r.  A source is never a destination: the copy runs in place.
// The relative weight the truncation loses is below N * 2^-40.
constexpr int RESAMPLE_THREADS = 256;
constexpr int RESAMPLE_MAX_MEMBERS = 1 << 23;
constexpr int RESAMPLE_COPY_BYTES = 16384;  // of a spin row per workgroup of the copy kernel: 256 threads x 4 x 16 bytes
// sga_resample's arguments, checked on the host before anything is enqueued: nullptr, or what is wrong with them.
// R local replicas of Rg, the first the global replica0; n_models > 1: Rg / n_models consecutive replicas per model.
inline const char *resample_check(int n_populations, const double *dbeta, int R, int Rg, int replica0, int n_models) {
    if (!dbeta) return "dbeta is NULL";
    if (R <= 0) return "no replicas";
    if (n_populations < 1) return "n_populations must be at least 1";
    if (R % n_populations != 0) return "n_populations does not divide the number of local replicas";
    const int N = R / n_populations;
    if (N > RESAMPLE_MAX_MEMBERS) return "a population holds more than 2^23 members (the weight sum would leave 64 bits)";
    for (int p = 0; p < n_populations; ++p)
        if (!(dbeta[p] - dbeta[p] == 0.0)) return "dbeta must be finite";  // (NaN and +-inf fail alike)
    if (replica0 % N != 0) return "a shard boundary lies inside a population (replica0 must be a multiple of the population size)";
    if (n_models > 1 && Rg > 0) {
        const long long reps = Rg / n_models;
        for (int p = 0; p < n_populations; ++p) {
            const long long first = (long long)replica0 + (long long)p * N;
            if (reps <= 0 || first / reps != (first + N - 1) / reps) return "a population lies across two models";
        }
    }
    return nullptr;
}
// bytes of the plan's scratch for R replicas in n_pop populations, and where its arrays lie in it (each 16-byte aligned)
struct ResampleScratch {
    size_t c, f, sp, parent, take, shift, sum, dbeta, bytes;
};
inline ResampleScratch resample_scratch(long long R, long long n_pop) {
    auto up = [](size_t v) { return (v + 15) / 16 * 16; };
    ResampleScratch s{};
    s.c = 0;
    s.f = s.c + up((size_t)R * 8);
    s.sp = s.f + up((size_t)R * 4);
    s.parent = s.sp + up((size_t)R * 4);
    s.take = s.parent + up((size_t)R * 4);
    s.shift = s.take + up((size_t)R * 4);
    s.sum = s.shift + up((size_t)n_pop * 8);
    s.dbeta = s.sum + up((size_t)n_pop * 8);
    s.bytes = s.dbeta + up((size_t)n_pop * 8);
    return s;
}
struct ResampleArgs {
    const double *energy;       // [R] tracked energies
    const double *best_energy;  // [R]
    const double *dbeta;        // [n_pop], on the device
    unsigned long long *C;      // [R] scratch: W_r, then the inclusive sums C_r
    int *F;                     // [R] scratch: children of members 0 ... r of r's population
    int *SP;                    // [R] scratch: surplus copies of members 0 ... r
    int32_t *parent;            // [R] out: LOCAL replica index of every slot's parent (d itself where it is not overwritten)
    int *take_best;             // [R] out: 1 where slot d is overwritten and its parent's energy is below d's best
    double *shift;              // [n_pop] out: x_max
    unsigned long long *sum;    // [n_pop] out: S
    int N, n_pop;
    uint32_t gpop0, seed_lo, seed_hi, round;  // gpop0 = replica0 / N: the global index of population 0
};
hipError_t launch_resample_plan(const ResampleArgs &a, hipStream_t st);
// For every slot d with parent[d] != d: the parent's spin row, its tracked energy (the bits), and, where take_best[d], the
// parent's state as d's best.  In place: no source row is a destination.
hipError_t launch_resample_copy(const int32_t *parent, const int *take_best, int8_t *spins, double *energy, int8_t *best_spins,
                                double *best_energy, int sstride, int R, hipStream_t st);

// Spin and link overlaps between pairs of replicas (pair_overlaps.hip; sga_get_pair_overlaps /
// sga_accumulate_ladder_overlaps / sga_get_link_count): one workgroup of 256 threads per pair.  d = the sites where the
// two replicas differ; with links asked for the diff words also go to a bitmap of ceil(n / 32) words in LDS, and groups
// of lanes walk the rows of cv counting the links (the entries cluster_moves_kernel follows: value not +-0, j != i,
// 0 <= j < n) whose two ends differ in x -- the broken links b.  Read only.
constexpr int PAIR_OVERLAP_THREADS = 256;
constexpr size_t PAIR_OVERLAP_LDS_FIXED = 64;  // wave sums of d (4 ints) and of b (4 64-bit words), in front of the bitmap
// the kernel's LDS: without links the fixed part alone
inline size_t pair_overlap_lds_bytes(long long n, bool links) {
    return PAIR_OVERLAP_LDS_FIXED + (links ? 4 * (size_t)((n + 31) / 32) : 0);
}
// the largest n whose diff bitmap (n / 8 bytes) fits the budget the cluster move allows itself: 1 308 160 sites
constexpr long long PAIR_OVERLAP_MAX_N = (long long)((CLUSTER_LDS_BUDGET - PAIR_OVERLAP_LDS_FIXED) / 4) * 32;
// Lanes that share one row, as log2: the smallest power of two that holds the layout's mean row (entries / n), from 1
// (a lane a row) to 64 (a wave a row).  A degree-6 lattice gets 8 lanes, a slotted layout of long rows a whole wave; a
// hub among short rows is walked by its few lanes in more steps.
inline int pair_overlap_group_log2(long long entries, long long n) {
    int g = 0;
    while (g < 6 && (long long)(1 << g) * n < entries) ++g;
    return g;
}
// The pair list of sga_get_pair_overlaps, checked on the host before anything is enqueued: nullptr, or what is wrong
// with it.  The call only reads: a replica may stand in many pairs, and a == b is a pair (d = b = 0).
inline const char *pair_overlap_pairs_check(const int32_t *pairs, int count, int R) {
    if (count < 0) return "count is negative";
    if (count > 0 && !pairs) return "pairs is NULL";
    for (int k = 0; k < 2 * count; ++k)
        if (pairs[k] < 0 || pairs[k] >= R) return "replica index out of range";
    return nullptr;
}
// The histogram arguments of sga_accumulate_ladder_overlaps (whether the buffers lie on the device is the caller's look)
inline const char *pair_overlap_hist_check(bool have_q, int bins_q, int q_shift, bool have_l, int bins_l, int l_shift) {
    if (!have_q) return "hist_q is NULL";
    if (bins_q < 1 || (have_l && bins_l < 1)) return "a histogram needs at least one bin";
    if (q_shift < 0 || q_shift > 31 || (have_l && (l_shift < 0 || l_shift > 31))) return "a bin shift lies outside [0, 31]";
    return nullptr;
}
struct PairOverlapArgs {
    const int8_t *spins;         // [R][sstride] the observed rows (current or best), sstride a multiple of 16
    const long long *rowptr64;   // [n + 1], links only
    const int2 *cv;              // (column, value bits), links only
    const int32_t *pairs;        // pair form: [count][2] local replicas
    const int32_t *slot_to_rep;  // ladder form (pairs == null): the slot map, [n_ladders][L] global ids
    int L, slot_lo, n_slots;     // ... pair p: ladders 2 (p / n_slots) and 2 (p / n_slots) + 1, slot slot_lo + p % n_slots
    int32_t *dist;               // pair form: [count] d, or null
    long long *broken;           // pair form: [count] b, or null
    unsigned long long *hist_q;  // ladder form: [count][bins_q], cell p bin min(d >> q_shift, bins_q - 1) grows by one
    unsigned long long *hist_l;  // ... [count][bins_l] of b, or null
    int bins_q, q_shift, bins_l, l_shift;
    int links;                   // b is asked for: the bitmap and the walk
    int group_log2;              // lanes to a row
    int n, sstride, R, count, replica0;
};
hipError_t launch_pair_overlaps(const PairOverlapArgs &a, hipStream_t st);
// *out += the number of links of the layout (out zeroed by the caller, on the device)
hipError_t launch_link_count(const long long *rowptr64, const int2 *cv, int n, int group_log2, unsigned long long *out,
                             hipStream_t st);

// Class-resolved overlaps between pairs of replicas (class_overlaps.hip; sga_get_class_overlaps /
// sga_accumulate_ladder_class_overlaps): one workgroup of 256 threads per pair, a lane a site, and per map m a counter
// cnt[m C + c] in LDS for D[m][c] = the differing sites of class c.  Read only.
//   copies: every one of the workgroup's four waves counts into a copy of its own where four copies fit the budget
//           (M C <= CLASS_OVERLAP_MAX_MC_4 = 10 224), else all four share one copy;
//   LDS:    4 bytes x copies x M C, nothing else;
//   bound:  M C <= CLASS_OVERLAP_MAX_MC = 40 896, one copy filling CLUSTER_LDS_BUDGET.
constexpr int CLASS_OVERLAP_THREADS = 256;
#ifndef SGA_CLASS_OVERLAP_MAX_COPIES  // (a measurement build passes 1: profiles/class_overlaps_timing.py)
#define SGA_CLASS_OVERLAP_MAX_COPIES 4
#endif
constexpr long long CLASS_OVERLAP_MAX_MC = (long long)(CLUSTER_LDS_BUDGET / 4);
constexpr long long CLASS_OVERLAP_MAX_MC_4 = (long long)(CLUSTER_LDS_BUDGET / 16);
inline int class_overlap_copies(long long mc) {
    return SGA_CLASS_OVERLAP_MAX_COPIES >= 4 && mc <= CLASS_OVERLAP_MAX_MC_4 ? 4 : 1;
}
inline size_t class_overlap_lds_bytes(long long mc) { return 4 * (size_t)class_overlap_copies(mc) * (size_t)mc; }
// The class-map arguments of both calls, checked on the host before anything is enqueued: nullptr, or what is wrong
// (SGA_ERR_INVALID).  n: the engine's row length in sites.
inline const char *class_overlap_args_check(bool have_classes, bool have_out, int n_maps, int n_classes, long long ld, long long n) {
    if (!have_classes) return "classes is NULL";
    if (!have_out) return "the output is NULL";
    if (n_maps < 1) return "n_maps must be at least 1";
    if (n_classes < 1) return "n_classes must be at least 1";
    if (ld < n) return "ld is smaller than n";
    return nullptr;
}
// ... and what is not served (SGA_ERR_UNSUPPORTED): more counters than LDS holds
inline const char *class_overlap_unsupported(int n_maps, int n_classes) {
    if ((long long)n_maps * (long long)n_classes > CLASS_OVERLAP_MAX_MC)
        return "class overlaps: n_maps * n_classes counters do not fit LDS (at most 40896)";
    return nullptr;
}
struct ClassOverlapArgs {
    const int8_t *spins;         // [R][sstride] the observed rows (current or best)
    const int32_t *pairs;        // pair form: [count][2] local replicas
    const int32_t *slot_to_rep;  // ladder form (pairs == null): the slot map, [n_ladders][L] global ids
    int L, slot_lo, n_slots;     // ... pair p: ladders 2 (p / n_slots) and 2 (p / n_slots) + 1, slot slot_lo + p % n_slots
    const int32_t *classes;      // [n_maps][ld]; a value outside [0, n_classes) is no class
    long long ld;
    int n_maps, n_classes;
    int vec_classes;             // set by the launcher: classes is 16-byte aligned and ld a multiple of 4 (int4 loads)
    int32_t *dist;               // pair form: [count][n_maps][n_classes] D
    unsigned long long *sum1;    // ladder form: [count][n_maps][n_classes], += D[m][c]
    unsigned long long *sum2;    // ... [count][n_maps][n_classes][n_classes], += D[m][c] D[m][c'], or null
    int n, sstride, R, count, replica0;
};
hipError_t launch_class_overlaps(const ClassOverlapArgs &a, hipStream_t st);

}  // namespace sga

#endif  // SGA_REPLICAS_H
