// sga_route.h -- WHICH kernel form sweeps a problem: pure functions of a sga_route_query (include/sga.h: the problem's
// traits as the set-time scans found them, replica count, tuning, options).  No device call anywhere in sga_route.cpp;
// the LDS-footprint helpers it uses (sga_kernels.h) are plain arithmetic on the kernels' layouts.  The engine asks
// these functions at the stage where each decision is latched (set / replicas / sweep); sga_explain_route strings the
// same calls together for tests.  The one decision that has a memory -- the cached-field modes' look at the acceptance
// counters -- is a transition on a plain struct (ReplicaRouting) from counters the engine hands in.
#ifndef SGA_ROUTE_H
#define SGA_ROUTE_H
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "sga.h"

namespace sga_impl {

inline thread_local std::string g_last_error;

inline int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

// ---- engine options (sga_set_option / sga_get_option, include/sga.h) ----------------------------------
// Form selection switches -- A/B measurements, parity tests that force the slower forms -- are per-engine
// values behind the C ABI.  The environment is consulted ONCE, in sga_create, for the defaults (the variable
// named here); nothing else in the library reads it.
enum Opt {
    OPT_LOOK_AHEAD, OPT_CLF_WAVES, OPT_SPARSE_ROUTE, OPT_BATCHED_ENERGY, OPT_FORCE_GENERAL, OPT_CSR_UPDATES_PER_STEP,
    OPT_TSP_PARALLEL, OPT_FORCE_CSR_BITS, OPT_CSR_BITS, OPT_CSR_SLOTS, OPT_HALF_TABLE, OPT_FORCE_CSR_ACC,
    OPT_FORCE_DENSE_CANON, OPT_ZERO_SLOT_EVERY, OPT_REPLICA_ROUTING, OPT_FIELDS_SCRATCH_MB, OPT_CLF_BATCHED,
    OPT_CLF_TAIL_WAVES, OPT_CLF_FIXED_POINT, OPT_ROW_SHARED, OPT_ROW_SHARED_GRID, OPT_ROW_SHARED_FIELDS,
    OPT_ROW_SHARED_TILE_SITES, OPT_ROW_SHARED_WINDOW, OPT_BATCH_FIXED_POINT, OPT_RAGGED_FIELD_CACHE, OPT_COUNT
};
struct OptDef {
    const char *key;
    const char *env;     // environment variable giving the default at sga_create (nullptr: none)
    int env_presence;    // 1: the variable being set means `env_value`; 0: its integer value is taken
    long long env_value;
    long long def, lo, hi;
    int stage = 0;       // where the value is latched: 0 = every sga_sweep, 1 = sga_init_replicas, 2 = sga_set_dense / sga_set_csr
};
constexpr OptDef OPT_DEFS[OPT_COUNT] = {
    {"look_ahead", "SGA_NO_LOOK_AHEAD", 1, 0, 1, 0, 1, 0},
    {"clf_waves", "SGA_CLF_WAVES", 0, 0, 0, 0, 16, 0},
    {"sparse_route", "SGA_NO_SPARSE_ROUTE", 1, 0, 1, 0, 1, 2},
    {"batched_energy", "SGA_NO_MFMA_ENERGY", 1, 0, 1, 0, 2, 0},
    {"force_general", "SGA_FORCE_GENERAL", 1, 1, 0, 0, 1, 0},
    {"csr_updates_per_step", "SGA_CSR_PAIR_AHEAD", 0, 0, -1, -1, 8, 0},
    {"tsp_updates_per_step", "SGA_TSP_PARALLEL", 0, 0, -1, -1, 8, 0},
    {"force_csr_bits", "SGA_FORCE_CSR_BIG", 1, 1, 0, 0, 1, 1},
    {"csr_bits", "SGA_NO_CSR_BITS", 1, 0, 1, 0, 1, 1},
    {"csr_slots", "SGA_NO_CSR_SLOTS", 1, 0, 1, 0, 1, 2},
    {"half_integer_table", "SGA_NO_HALF_TABLE", 1, 0, 1, 0, 1, 2},
    {"force_csr_acc", "SGA_FORCE_CSR_ACC", 0, 0, 0, 0, 3, 2},
    {"force_dense_canonical", "SGA_FORCE_DENSE_CANON", 1, 1, 0, 0, 1, 2},
    {"zero_slot_every", "SGA_ZERO_SLOT_EVERY", 0, 0, 0, 0, 1ll << 21, 2},
    {"replica_routing", "SGA_NO_REPLICA_ROUTING", 1, 0, 1, 0, 1, 0},
    {"fields_scratch_mb", "SGA_FIELDS_SCRATCH_MB", 0, 0, 256, 1, 65536, 0},
    {"clf_batched", "SGA_CLF_BATCHED", 0, 0, 2, 0, 2, 0},
    {"clf_tail_waves", "SGA_NO_CLF_TAIL_WAVES", 1, 0, 1, 0, 1, 0},
    {"clf_fixed_point", nullptr, 0, 0, 0, 0, 1, 2},
    {"row_shared", "SGA_ROW_SHARED", 0, 0, 2, 0, 2, 0},
    {"row_shared_grid", "SGA_ROW_SHARED_GRID", 0, 0, 0, 0, 1, 0},
    {"row_shared_fields", "SGA_ROW_SHARED_FIELDS", 0, 0, 2, 0, 2, 0},
    {"row_shared_tile_sites", "SGA_ROW_SHARED_TILE_SITES", 0, 0, 0, 0, 4096, 0},
    {"row_shared_window", "SGA_ROW_SHARED_WINDOW", 0, 0, 0, 0, 1024, 0},
    // ("ragged_field_cache" stays the last entry and the list ends row_shared_window, batch_fixed_point, ragged_field_cache;
    //  queries name options by key -- _native.route_query, tests/golden/route_table.json -- never by number)
    {"batch_fixed_point", "SGA_BATCH_FIXED_POINT", 0, 0, 0, 0, 1, 2},
    {"ragged_field_cache", nullptr, 0, 0, 0, 0, 1, 2},
};
inline int find_option(const char *key) {
    if (!key) return -1;
    for (int i = 0; i < OPT_COUNT; ++i)
        if (std::strcmp(key, OPT_DEFS[i].key) == 0) return i;
    return -1;
}
static_assert(OPT_COUNT <= SGA_ROUTE_MAX_OPTS, "sga_route_query::opt holds every option");

}  // namespace sga_impl

namespace sga_windows {
struct WindowTraits;  // sga_windows.h
}

namespace sga_route {

using Query = sga_route_query;

// ---- set time ---------------------------------------------------------------------------------------------------
// A sparse matrix handed over dense (sga_set_dense, SGA_J_AUTO) is taken as CSR: asked before the rows are counted ...
bool sparse_route_wanted(int storage_requested, int n_models, int n, bool j_integer, int field_cache, bool clf_problem,
                         long long opt_sparse_route);
// ... and decided once they are (longest row, total entries)
bool sparse_route_taken(long long longest_row, long long total_entries);
// CSR rows padded to whole 64-entry slots at set time (the problems that run the wide forms)
bool csr_slots_at_set(long long nnz, int n, long long opt_csr_slots);

// ---- dense geometry (latched with the replicas; re-evaluated when the tuning changes) -----------------------------
struct DenseGeometry {
    int waves = 0, cpw = 0;        // what sga_describe reports (bit-plane form: the int8 fallback's 8 x (Wb * Cb))
    int waves_t2 = 0, cpw_t2 = 0;  // bit-plane form
    long long ld = 0;              // spins per replica (whole chunks)
    bool fits = true;              // replica spins (+ accept table) fit LDS
};
bool choose_geometry(int n, int epc, int R, int forced_waves, int &W, int &CPW, int max_cpw, int unit);
DenseGeometry dense_geometry(const Query &q);
long long dense_ldj(const Query &q);  // row stride of the packed couplings, elements

// ---- CSR forms ------------------------------------------------------------------------------------------------------
bool csr_rows_medium(const Query &q);       // rows of 65 ... 256 entries on the four-updates-per-step form
int csr_updates_per_step(const Query &q);   // 0 | 1 | 2 | 4 | 8
struct CsrForm {
    bool bits = false;        // spins as bits in LDS
    int big_form = 0;         // 0 int8 spins | 1 bits, one replica per workgroup (64-bit extents, slots) | 2 bits, narrow
    int waves = 1;            // waves per replica
    int sstride = 0;
    int table_m = 0;          // (dropped to 0 where the table does not fit LDS)
    bool needs_slots = false; // the form addresses rows by 64-entry slots
    bool wants_packed = false;// one dword per entry where the values allow
    const char *error = nullptr;  // the problem does not fit any form
};
CsrForm csr_replica_form(const Query &q);
int csr_replicas_per_block(const Query &q, const CsrForm &f);
// ragged CSR batches (sga_set_csr_batch; a query with n_models > 1): the narrow one-update int8 form, or an error
// naming the option that would pick another form
CsrForm csr_ragged_form(const Query &q);
// one set of rows under n_models field vectors (sga_set_csr_shared; a CSR query with n_models > 1 and shared_j): the
// one-model decision restricted to one wave per replica (int8 spins, or bit spins with several replicas per workgroup),
// or an error starting "shared-coupling CSR batches"
CsrForm csr_shared_form(const Query &q);
// the kernel family launch_sweep_csr takes for production arguments: "rows" | "narrow" | "narrow-bits" | "wide-bits" | "wide-bytes"
const char *csr_kernel_family(const Query &q, const CsrForm &f, bool slotted_now);

// ---- TSP-structured couplings --------------------------------------------------------------------------------------
struct TspForm {
    int waves = 1, passes = 1;
};
TspForm tsp_form(int npad, int tune_waves);

// ---- couplings as a sum of complete graphs on groups (sga_set_groups) ---------------------------------------------
struct GroupsForm {
    int waves = 1;            // waves per replica of the production form (the general form runs one)
    int sstride = 0;
    bool wide = false;        // group sums as int32 (a group of 2^15 members or more)
    size_t lds_bytes = 0;
    const char *error = nullptr;  // spin bits and group sums do not fit LDS
};
GroupsForm groups_form(const Query &q);

// ---- cached local fields (sga_set_field_cache) ------------------------------------------------------------------------
// nullptr when the cached-field sweep can serve q (with q.sstride / q.ldj as laid out), else the reason
const char *clf_refusal(const Query &q);
bool dense_fixed_point(const Query &q);     // a dense query served by the fixed-point cached-field form (clf_bits 32 | 64)
double routing_theta(const Query &q);       // break-even acceptance of one replica between the two kernel families
bool auto_starts_cached(const Query &q);    // SGA_FIELD_CACHE_AUTO before any acceptance is known
int clf_csr_waves(const Query &q);          // waves per replica of the cached-field sweep over CSR couplings
// ---- sweep time ------------------------------------------------------------------------------------------------------
int sweeps_per_launch(const Query &q, int n_sweeps, int tune_spl, int npad_tsp);

// Which looks at the per-replica acceptance counters a cached-field sweep of q takes when a call starts (meaningful
// where clf_refusal(q) == nullptr).
struct ClfLooks {
    bool is_auto = false;     // SGA_FIELD_CACHE_AUTO: replicas move between the two kernel families
    bool tail = false;        // option "clf_tail_waves" on, "clf_waves" left to the library, dense couplings -- and, with
                              // `sized`, a launch large enough for eight waves per replica to matter
    bool adaptive = false;    // option "clf_batched" = 2: several accepts per round while the hottest replica is hot
    bool any() const { return is_auto || tail || adaptive; }
};
// sized = false is what the walk of a long call in 16-sweep pieces asks (so that the form follows the run): that test
// has never applied the size conditions of the tail look (it predates them) -- a call with the look enabled but too
// small for it is still cut, which changes how the run divides into launches, not the chain.  Kept as it is.
ClfLooks clf_looks(const Query &q, bool sized = true);

// What the policy knows about the replicas of an engine between calls.
struct ReplicaRouting {
    std::vector<int> route;          // per local replica: 0 = cached-field kernel, 1 = row-per-proposal kernel (AUTO)
    int n_cached = 0;                // replicas routed to the cached-field kernel
    bool wide = false;               // the cached-field launch runs at eight waves per replica (option "clf_tail_waves")
    bool hot = true;                 // its hottest replica accepts > ~1 %: several accepts per round (option "clf_batched" = 2)
    bool dirty = true;               // the device copy of the replica lists is stale
    bool unavailable = false;        // the fields could not be allocated: AUTO stays on the row-per-proposal kernels
    std::vector<unsigned long long> mark_acc;  // per-replica acceptance counters at the last look
    long long mark_attempted = 0;    // per-replica attempts at the last look
    int interval = 4;                // sweeps until the next look (doubles up to 16)
    void reset() { *this = ReplicaRouting{}; }
};
struct LookInput {
    int n = 0, R = 0;                // spins (ragged batches: the largest model's), local replicas
    long long attempted = 0;         // per-replica attempts so far
    const int *spins = nullptr;      // [R] spins of each replica's model (ragged batches), nullptr: n each
    double theta = 0.0;              // routing_theta(q)
    bool start_cached = true;        // the routes before anything is known: all cached (ON; AUTO: auto_starts_cached(q))
    ClfLooks looks;
    bool per_replica = true;         // option "replica_routing" != 0 and dense couplings
};
// The policy's step when a call starts.  New replica count: the initial routes.  A look is due after `interval` sweeps
// of attempts (or when the attempts counter went backwards); only then read_counters is called, once, for the [R]
// acceptance counters now (nullptr: the read failed, nothing moves), and the routes, hot / wide, the marks and the
// interval move.  True: somebody returns from the row kernels, the resident fields are to be seeded anew.
bool look(ReplicaRouting &s, const LookInput &in, const std::function<const unsigned long long *()> &read_counters);

// A dense query as the traits the window forms' admission rules read (sga_windows.h); what a query does not carry is
// assumed there, line by line.  explain() prints " sweep=row-shared(...)" from it.
sga_windows::WindowTraits window_traits_of_query(const Query &q);

std::string explain(const Query &q);

}  // namespace sga_route

#endif  // SGA_ROUTE_H
