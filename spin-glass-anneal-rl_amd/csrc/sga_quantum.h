// sga_quantum.h -- simulated quantum annealing: the Trotter-slice geometry and the admission rules of its calls,
// sga_sweep_transverse (sweep_transverse.hip), sga_sweep_transverse_dense (sweep_transverse_clf.hip, sweep_transverse_fx.hip),
// sga_worldline_clusters (worldline_clusters.hip), sga_worldline_clusters_dense (worldline_clusters_dense.hip),
// sga_get_time_links and sga_exchange_transverse (trotter_exchange.hip).  The pure half: no sga_engine and no HIP call, so
// tests/c_abi/transverse_plan.cpp, transverse_dense_plan.cpp, transverse_fx_plan.cpp, worldline_plan.cpp,
// worldline_dense_plan.cpp and trotter_exchange_plan.cpp pin it on the CPU.  The engine half is sga_quantum.cpp: it reads an engine into a
// TrotterProblem and runs the calls.
//
// The local replicas are G = R_local / P contiguous groups of P slices, slice p of group g in row g P + p; replica0 is a
// multiple of P, so p is the global slice index too.  The slices of a group form a ring.
#ifndef SGA_QUANTUM_H
#define SGA_QUANTUM_H
#include <cstdio>
#include "sga_kernels.h"

namespace sga {

// ---- the geometry ---------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int slice_row(int g, int P, int p) { return g * P + p; }
__host__ __device__ __forceinline__ int ring_next(int p, int P) { return p + 1 == P ? 0 : p + 1; }
__host__ __device__ __forceinline__ int ring_prev(int p, int P) { return p == 0 ? P - 1 : p - 1; }
// A HALF-SWEEP moves the P / 2 slices of one parity of every group (P even: both neighbours of a moving slice stand
// still).  The moving slice of index m in [0, G P / 2): its group, its row and its two neighbours' rows.
struct MovingSlice {
    int g, r, up, dn;
};
__host__ __device__ __forceinline__ MovingSlice moving_slice(int m, int P, int parity) {
    const int half = P >> 1;
    MovingSlice o;
    o.g = m / half;
    const int p = 2 * (m - o.g * half) + parity;
    o.r = slice_row(o.g, P, p);
    o.up = slice_row(o.g, P, ring_next(p, P));
    o.dn = slice_row(o.g, P, ring_prev(p, P));
    return o;
}

// ---- LDS --------------------------------------------------------------------------------------------------------------------
// The CSR sweep: one wave per moving slice, its int8 spins in LDS (sstride bytes a wave).
constexpr size_t TRANSVERSE_LDS_BUDGET = 160 * 1024 - 256;
inline int transverse_waves_per_block(int sstride) {  // 0: a slice's spins do not fit
    if (sstride <= 0) return 0;
    const size_t wpb = TRANSVERSE_LDS_BUDGET / (size_t)sstride;
    return wpb > (size_t)CSR_WAVES_PER_BLOCK ? CSR_WAVES_PER_BLOCK : (int)wpb;
}
// The dense sweep: one workgroup per moving slice, LDS = fields [ldf] int16 | int32, the slice's spin bits, the two
// neighbour slices' spin bits (n / 4 bytes), the decision slots -- 2.375 n bytes with int16 fields, 4.375 n with int32
// fields, plus padding and 512 bytes of slots.  On fixed-point fields (sweep_transverse_fx.hip) they are int32 | int64:
// 4.375 n | 8.375 n.
constexpr size_t TRANSVERSE_DENSE_SLOT_BYTES = 2 * 8 * 8 * sizeof(int);  // [2][CLF_MAX_WAVES][CLF_SLOT_INTS]
__host__ __device__ constexpr long long transverse_dense_bits_bytes(int sstride) { return (sstride / 8 + 15) & ~15; }
inline size_t transverse_dense_lds_bytes(long long ldf, int fbytes, int sstride) {
    return (size_t)((ldf * fbytes + 15) & ~15ll) + 3 * (size_t)transverse_dense_bits_bytes(sstride) + TRANSVERSE_DENSE_SLOT_BYTES;
}
// The clusters: one wave per group, lane p = slice p; the group's spins as one word per site, bit p = [s_p[i] < 0]:
// uint32_t for P <= 32, uint64_t beyond.  Behind the words lie 64 int32 accumulators of the segment sums.
constexpr int WORLDLINE_MAX_SLICES = 64;
constexpr size_t WORLDLINE_ACC_BYTES = 64 * sizeof(int32_t);
inline int worldline_word_bytes(int n_slices) { return n_slices <= 32 ? 4 : 8; }
// the words of a group: n rounded up to the 4 sites of a dword of int8 spins (the transposes move 4 sites a step)
inline size_t worldline_lds_bytes(int n, int n_slices) {
    return (((size_t)(n > 0 ? n : 0) + 3) / 4) * 4 * (size_t)worldline_word_bytes(n_slices) + WORLDLINE_ACC_BYTES;
}
inline int worldline_max_sites(int n_slices) {  // the largest n a group of n_slices slices is served at
    return (int)((TRANSVERSE_LDS_BUDGET - WORLDLINE_ACC_BYTES) / (size_t)worldline_word_bytes(n_slices) / 4 * 4);
}
// the threshold a bond's 24 random bits are held against: floor(p 2^24) in double, p = 1 -> 2^24 (every bond active)
inline uint32_t worldline_threshold(double p_bond) { return (uint32_t)(long long)(p_bond * 16777216.0); }

// ---- admission ------------------------------------------------------------------------------------------------------------
// What of an engine the admission rules read.
struct TrotterProblem {
    int n = 0, R_local = 0, replica0 = 0, sstride = 0;
    int csr = 0, tsp = 0, groups = 0, ragged = 0, n_models = 1;
    int metropolis = 1;  // the engine's rule is SGA_RULE_METROPOLIS (the sweeps; the clusters bring their own rule)
    // sparse couplings (the CSR sweep, the clusters)
    int csr_acc = CSR_ACC_F64_CANON;
    int consistent_dE = 1;  // J symmetric with zero diagonal: the rule's dE is the energy change
    // dense couplings (the dense sweep)
    int clf_problem = 0;            // the one-model integer cached-field form admits the problem (set-time scan)
    const char *clf_why = nullptr;  // ... where it does not: which condition failed
    int field_bits = 16;            // 16 | 32: the width of the resident fields
    long long ldf = 0;              // elements of a replica's field row
    // ... on fixed-point fields (option "clf_fixed_point": the dense problems clf_problem does not take)
    int fx_bits = 0;               // 32 | 64: the fixed-point form admits the problem, D = 2^k J s in that width; 0: it does not
    const char *fx_why = nullptr;  // the fixed-point verdict's refusal, where the option is on and it refused
    // the exchange between groups
    int R_global = 0;  // the replicas of every rank
};
// The argument errors of a call (SGA_ERR_INVALID), the same ladder for all four: they come first, so that a wrong call is
// told so whatever the problem.  What differs between the calls comes in: the text for a NULL array, whether arith was
// acceptable (a call without one: true), the call's own rule on n_slices as its verdict, and the test of a value.
// values: the caller's HOST array [n_sweeps][R_local / n_slices].
template <typename T, typename Ok>
inline const char *trotter_argument_error(bool have_engine, const TrotterProblem &p, int n_sweeps, int n_slices, const T *values,
                                          const char *values_null, bool arith_ok, const char *slices_refused, Ok value_ok,
                                          const char *value_refused) {
    if (!have_engine) return "engine is NULL";
    if (!values) return values_null;
    if (p.n <= 0) return "no couplings set";
    if (p.R_local <= 0) return "no replicas (call sga_init_replicas)";
    if (n_sweeps < 0) return "n_sweeps < 0";
    if (!arith_ok) return "bad arith";
    if (n_slices < 2) return "n_slices must be at least 2";
    if (slices_refused) return slices_refused;
    if (p.R_local % n_slices != 0) return "n_slices must divide the number of local replicas";
    if (p.replica0 % n_slices != 0) return "replica0 must be a multiple of n_slices (groups lie whole on a rank)";
    const long long count = (long long)n_sweeps * (p.R_local / n_slices);
    for (long long i = 0; i < count; ++i)
        if (!value_ok(values[i])) return value_refused;
    return nullptr;
}
// ... of the two sweeps: k_perp finite, an even number of slices
inline const char *sweep_argument_error(bool have_engine, const TrotterProblem &p, int n_sweeps, int n_slices, bool arith_ok,
                                        const float *k_perp) {
    return trotter_argument_error(have_engine, p, n_sweeps, n_slices, k_perp, "k_perp is NULL", arith_ok,
                                  n_slices % 2 != 0 ? "n_slices must be even (a moving slice never has a moving neighbour)" : nullptr,
                                  [](float k) { return k - k == 0.0f; }, "k_perp holds a NaN or an infinite value");
}
// The kinds of problem no call serves (SGA_ERR_UNSUPPORTED); what: the call's noun.  The text stands in a buffer of the
// calling thread until that thread asks again.
inline const char *trotter_kind_refused(const TrotterProblem &p, const char *what) {
    const char *kind = p.tsp            ? "sga_set_tsp problems"
                       : p.groups       ? "sga_set_groups / sga_set_groups_csr problems"
                       : p.ragged       ? "ragged CSR batches"
                       : p.n_models > 1 ? "many-model batches (shared or stacked)"
                                        : nullptr;
    if (!kind) return nullptr;
    static thread_local char text[160];
    std::snprintf(text, sizeof(text), "%s are not implemented for %s", what, kind);
    return text;
}

// The admission rules, pure functions: nullptr where the call is served, else why not, with *invalid = true for
// SGA_ERR_INVALID and false for SGA_ERR_UNSUPPORTED.  The argument errors, the kinds, then what the call's own kernel asks.
inline const char *transverse_check(bool have_engine, const TrotterProblem &p, int n_sweeps, int n_slices, bool arith_ok,
                                    const float *k_perp, bool *invalid) {
    *invalid = true;
    if (const char *why = sweep_argument_error(have_engine, p, n_sweeps, n_slices, arith_ok, k_perp)) return why;
    *invalid = false;
    if (const char *why = trotter_kind_refused(p, "transverse sweeps")) return why;
    if (!p.csr) return "transverse sweeps need sparse (CSR) couplings: dense couplings are not served";
    if (p.csr_acc != CSR_ACC_F32_TABLE && p.csr_acc != CSR_ACC_F32)
        return "transverse sweeps need integer couplings with exact fp32 row sums (real-valued J needs the canonical order)";
    if (!p.metropolis) return "transverse sweeps are implemented for the Metropolis rule only";
    if (!p.consistent_dE) return "transverse sweeps need symmetric couplings with a zero diagonal";
    if (transverse_waves_per_block(p.sstride) < 1) return "transverse sweeps: a slice's int8 spins do not fit LDS";
    return nullptr;
}
// (the bound on n of include/sga.h is the last test: the fields, three rows of spin bits and the slots within the budget)
inline const char *transverse_dense_check(bool have_engine, const TrotterProblem &p, int n_sweeps, int n_slices, bool arith_ok,
                                          const float *k_perp, bool *invalid) {
    *invalid = true;
    if (const char *why = sweep_argument_error(have_engine, p, n_sweeps, n_slices, arith_ok, k_perp)) return why;
    *invalid = false;
    if (const char *why = trotter_kind_refused(p, "dense transverse sweeps")) return why;
    if (p.csr) return "dense transverse sweeps need dense rows: the engine holds sparse (CSR) couplings, which sga_sweep_transverse serves";
    const bool fx = !p.clf_problem && (p.fx_bits == 32 || p.fx_bits == 64);  // (the integer form keeps what it takes)
    if (!p.clf_problem && !fx) {
        if (p.fx_why) return p.fx_why;  // (option "clf_fixed_point" is on and its verdict refused the problem)
        return p.clf_why ? p.clf_why : "dense transverse sweeps need the integer cached-field form (integer symmetric J, zero diagonal)";
    }
    if (!p.metropolis) return "dense transverse sweeps are implemented for the Metropolis rule only";
    const int bits = fx ? p.fx_bits : p.field_bits;  // the width of the fields the launch keeps in LDS
    if ((!fx && bits != 16 && bits != 32) || p.sstride <= 0 || p.ldf <= 0 ||
        transverse_dense_lds_bytes(p.ldf, bits / 8, p.sstride) > TRANSVERSE_LDS_BUDGET)
        return "dense transverse sweeps: a slice's fields, spin bits and neighbour bits do not fit LDS";
    return nullptr;
}
// (p_bond in [0, 1]; at most one lane of a wave per slice; the engine's rule is not looked at)
inline const char *worldline_argument_error(bool have_engine, const TrotterProblem &p, int n_sweeps, int n_slices, const double *p_bond) {
    return trotter_argument_error(have_engine, p, n_sweeps, n_slices, p_bond, "p_bond is NULL", true,
                                  n_slices > WORLDLINE_MAX_SLICES ? "n_slices must be at most 64 (one lane of a wave per slice)" : nullptr,
                                  [](double b) { return b >= 0.0 && b <= 1.0; }, "p_bond holds a NaN or a value outside [0, 1]");
}
inline const char *worldline_check(bool have_engine, const TrotterProblem &p, int n_sweeps, int n_slices, const double *p_bond,
                                   bool *invalid) {
    *invalid = true;
    if (const char *why = worldline_argument_error(have_engine, p, n_sweeps, n_slices, p_bond)) return why;
    *invalid = false;
    if (const char *why = trotter_kind_refused(p, "world-line clusters")) return why;
    if (!p.csr) return "world-line clusters need sparse (CSR) couplings: dense couplings are not served";
    if (p.csr_acc != CSR_ACC_F32_TABLE && p.csr_acc != CSR_ACC_F32)
        return "world-line clusters need integer couplings with exact fp32 row sums (real-valued J needs the canonical order)";
    if (!p.consistent_dE) return "world-line clusters need symmetric couplings with a zero diagonal";
    if (transverse_waves_per_block(p.sstride) < 1) return "world-line clusters: a slice's int8 spins do not fit LDS";
    if (p.n > worldline_max_sites(n_slices)) return "world-line clusters: a group's spin words do not fit LDS";
    return nullptr;
}
// (the argument ladder of worldline_check; the rule is not looked at; the kernel keeps nothing of size n in LDS: no bound on n)
inline const char *worldline_dense_check(bool have_engine, const TrotterProblem &p, int n_sweeps, int n_slices, const double *p_bond,
                                         bool *invalid) {
    *invalid = true;
    if (const char *why = worldline_argument_error(have_engine, p, n_sweeps, n_slices, p_bond)) return why;
    *invalid = false;
    if (const char *why = trotter_kind_refused(p, "dense world-line clusters")) return why;
    if (p.csr) return "dense world-line clusters need dense rows: the engine holds sparse (CSR) couplings, which sga_worldline_clusters serves";
    if (!p.clf_problem)
        return p.clf_why ? p.clf_why : "dense world-line clusters need the integer cached-field form (integer symmetric J, zero diagonal)";
    if (p.field_bits != 16 && p.field_bits != 32) return "dense world-line clusters: the resident fields are neither int16 nor int32";
    return nullptr;
}

// The broken time links of every group: the ladder with any P >= 2, odd ones included, and no value to read; then the
// kinds.  No coupling is read: dense rows in any storage, CSR rows of any class and every rule are served.
inline const char *time_links_check(bool have_engine, const TrotterProblem &p, int n_slices, const int64_t *links, bool *invalid) {
    *invalid = true;
    if (const char *why = trotter_argument_error(have_engine, p, 0, n_slices, links, "links is NULL", true, nullptr,
                                                 [](int64_t) { return true; }, nullptr))
        return why;
    *invalid = false;
    return trotter_kind_refused(p, "time links");
}
// One exchange round between neighbouring groups: the ladder over the G values of k_perp (one row), the parity, every
// group on this rank; then the kinds.
inline const char *exchange_check(bool have_engine, const TrotterProblem &p, int n_slices, const float *k_perp, int parity, bool *invalid) {
    *invalid = true;
    if (const char *why = trotter_argument_error(have_engine, p, 1, n_slices, k_perp, "k_perp is NULL", true, nullptr,
                                                 [](float k) { return k - k == 0.0f; }, "k_perp holds a NaN or an infinite value"))
        return why;
    if (parity != 0 && parity != 1) return "parity must be 0 or 1";
    if (p.R_local != p.R_global) return "exchanges between groups need every group on this rank (R_local == R_global)";
    *invalid = false;
    return trotter_kind_refused(p, "transverse-field exchanges");
}

// ---- the launches -----------------------------------------------------------------------------------------------------------
// One half-sweep of either sweep.
struct TrotterLaunch {
    const float *k_perp;  // device [G]: this sweep's coupling per group
    int n_slices;         // P
    int parity;           // the slices p with p % 2 == parity move
    int moving;           // G P / 2 waves (CSR) | workgroups (dense)
};
// a: the arguments of one production sweep (n_sweeps = 1, sweep0 = the sweep's counter); reads a.rowptr64 / a.cv
hipError_t launch_sweep_transverse(const SweepArgs &a, const TrotterLaunch &t, hipStream_t st);
// ... with the resident fields (fields, ldf, field_bits, field_scale) and the dense rows (J, ldj); the launch reads and
// writes the moving slices' fields
hipError_t launch_sweep_transverse_dense(const SweepArgs &a, const TrotterLaunch &t, bool j_is_i8, int waves, hipStream_t st);
// ... on fixed-point fields (sweep_transverse_fx.hip): a.fields = D = 2^k J s, a.field_bits = 32 | 64, a.field_scale = k >= 0;
// fp32 rows, or int8 rows (integer J, k = 0, int32 fields)
hipError_t launch_sweep_transverse_dense_fx(const SweepArgs &a, const TrotterLaunch &t, bool j_is_i8, int waves, hipStream_t st);
struct WorldlineArgs {
    const uint32_t *thr;  // device [n_sweeps][G]
    long long *stats;     // device [G][3], zeroed: segments formed, segments flipped, slice spins flipped (or null)
    int n_slices;         // P
    int n_sweeps;
    uint32_t round;       // sweep kk draws at round + kk
};
// a: the engine's CSR view, replica state and seed (a.n_sweeps, a.sweep0 unused); one launch serves the whole call
hipError_t launch_worldline_clusters(const SweepArgs &a, const WorldlineArgs &w, hipStream_t st);
// ... on the dense rows (J, ldj) and the resident fields (fields, ldf, field_bits, field_scale) of every slice, which the
// launch reads and writes: they stay valid.  waves per group: worldline_dense_waves (forced: option "clf_waves", 0 = none)
int worldline_dense_waves(long long ldj, bool j_is_i8, int forced);
hipError_t launch_worldline_clusters_dense(const SweepArgs &a, const WorldlineArgs &w, bool j_is_i8, int waves, hipStream_t st);

// The exchange between groups along the transverse field (trotter_exchange.hip).
constexpr int TIME_LINKS_CHUNK_SITES = 64 * 16;  // the sites of one workgroup of the count: one wave, 16 bytes a lane
// links[g] += the broken time links of group g, links [R / n_slices] ZEROED by the caller (device); spins [R][sstride]
// int8 with a zero pad, sstride a multiple of 16.  Exact integer atomics: the same in any order.
hipError_t launch_time_links(const int8_t *spins, int sstride, int R, int n_slices, long long *links, hipStream_t st);
struct TrotterExchangeArgs {
    const float *k_perp;     // device [G]
    const long long *links;  // device [G]: B of every group, as launch_time_links left it
    int *flags;              // device [G]: 1 for both groups of a swapped pair, else 0 (the decision writes every entry)
    int n_slices;            // P
    int parity;              // the pairs (a, a + 1) with a % 2 == parity
    uint32_t round;
    void *fields;            // the resident field rows, traded with the spins -- or null: not valid, left alone
    long long field_row_bytes;  // a multiple of 16
};
// a: the replica state and the seed (a.spins, a.energy, a.rep_temp, a.sstride, a.R, a.seed_lo, a.seed_hi).  The decision
// reads the energies the swap overwrites: two launches.
hipError_t launch_trotter_exchange_decide(const SweepArgs &a, const TrotterExchangeArgs &x, hipStream_t st);
hipError_t launch_trotter_exchange_swap(const SweepArgs &a, const TrotterExchangeArgs &x, hipStream_t st);

}  // namespace sga

#endif  // SGA_QUANTUM_H
