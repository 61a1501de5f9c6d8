// sga_windows.h -- the window forms of the dense sweep: row-shared windows (sweep_dense_rs.hip, option "row_shared"),
// their fields in tiles of sites (option "row_shared_fields") and sequential windows (sweep_dense_seq.hip,
// sga_set_sequential_windows).  Two halves.  The pure half answers WHETHER a problem admits a form and in which class,
// as functions of a plain WindowTraits: no sga_engine and no HIP call, so tests/c_abi/window_forms.cpp pins it on the
// CPU; sga_route::explain asks it through an adapter from sga_route_query (sga_route.cpp, window_traits_of_query).  The
// engine half (sga_engine_impl.h, "---- sga_windows.cpp") reads the traits off an engine, owns the forms' scratch and
// resident copies, and plans the forms of one sga_sweep call.
#ifndef SGA_WINDOWS_H
#define SGA_WINDOWS_H
#include "sga.h"
#include "sga_kernels.h"

namespace sga_windows {

// ---- the pure half ----------------------------------------------------------------------------------------------------
struct WindowTraits {
    // the problem, as the set-time scans found it
    bool dense = false, implicit = false, ragged = false;
    int n_models = 1;
    bool shared_j = false;
    int n = 0, R = 0;
    long long ldj = 0;
    int sstride = 0;
    bool want_i8 = false, acc64 = false;
    int table_m = 0, j_abs_max = 0;
    int grid_planes = 0, grid_k = 0;  // the set-time grid verdict (sga_classify.cpp, row_shared_grid; planes 0: none)
    bool consistent_dE = true;        // J symmetric with a zero diagonal
    bool packed = false;              // the packed rows exist
    int rule = SGA_RULE_METROPOLIS, field_cache = SGA_FIELD_CACHE_OFF, cus = 256;
    // options "row_shared", "row_shared_grid", "row_shared_window", "row_shared_fields", "row_shared_tile_sites",
    // "look_ahead", "force_general" (the values: the defaults are OPT_DEFS', sga_route.h)
    long long row_shared = 0, row_shared_grid = 0, row_shared_window = 0, row_shared_fields = 0, row_shared_tile_sites = 0;
    long long look_ahead = 0, force_general = 0;
    // the autotuner's window and the rule it was timed under, its geometry trials running, sga_set_sequential_windows
    int tuned_w = 0, tuned_rule = SGA_RULE_METROPOLIS;
    bool suspend = false;
    int seq_w = 0;
    // the tiles: resident planes exist, every off-diagonal |2^k J_ij| is 1, the runtime refused the tile kernel's LDS
    bool planes_resident = false, ones = false, tiles_refused = false;
    int groups = 0;  // sga_set_replica_groups: 0 the rule's choice, 1 | 2 | 4 forced
};

// The class of exact products a problem falls in.  why: null, or why there is none.
struct WindowClass {
    const char *why = nullptr;
    int planes = 0;  // magnitude planes of |2^k J| (1 | 3 | 8; 0: an integer |J| beyond 255)
    int grid = 0;    // 0 the integer class, else 1 + k: J on the grid 2^-k
    int jmax = 0;    // bound on |2^k J_ij|: j_abs_max for the integer class, 7 | 255 by the planes of the grid
};
// The ONE statement of the class choice: the integer class of the look-ahead form (the accept table's: integer J and h
// with exact fp32 sums), else -- option "row_shared_grid" = 1 -- the set-time grid verdict (J on 2^-k, scaled row sums
// below 2^24, any finite h; integer J beside a half-integer or real h is k = 0).
WindowClass form_class(const WindowTraits &t);
// What both forms ask of a problem and its replicas before anything of their own: one dense matrix (one model, or the
// models of sga_set_dense_shared, whose traits are the batch's; a stacked batch has a row i per model), symmetric with a
// zero diagonal (a flip's correction is read from the flipped site's row), a single-site rule, cache off, the general
// kernels not forced, R n below 2^31 (entries and bases are indexed in 32 bits), and a class.  why: the first that fails.
WindowClass admission(const WindowTraits &t);

// Row-shared windows: the window W for sweeps whose arguments are the production ones (lean: Philox sites, fp64 rule,
// no per-update traces), 0 where today's row-per-proposal kernel runs.  Beyond admission(): |J| <= 255 (bit-planes of
// |J|), the look-ahead form allowed, fewer than 2^20 replicas.  Metropolis decides with the accept table, Glauber and heat
// bath with the row kernels' general rule on the same exact fields (lean then implies SGA_ARITH_F64: sga_sweep refuses
// them fp32); the grid class decides with the general rule under every rule.
// Option "row_shared": 1 = wherever it applies (W: option "row_shared_window", else the autotuner's, else 1024), 2 = where
// sga_autotune measured it ahead (default).  The autotuner's W counts only while the rule is the one it was timed
// under: the form's time follows the flip rate, and Glauber's is not Metropolis'.
int row_shared_w(const WindowTraits &t, bool lean);
// Sequential windows as a SGA_SITE_SEQUENTIAL sweep without per-update traces would run them, W = 0 where the
// row-per-proposal kernel runs.  The product: int8 rows on the int8 matrix cores; fp32 rows too where every |2^k J_ij| <=
// 127 (through a resident int8 copy) -- else the fp32 cores.  The mode returned for fp32 rows is the class's; the sweep
// moves mode 0 to mode 1 where the copy cannot be had.  base and j8 are left null: they are the engine's.
sga::SeqWindows sequential(const WindowTraits &t);
// The fields kernel of the row-shared windows over resident planes, by option "row_shared_fields": the tile size S and
// whether the rows are sign-only, or S = 0 and the reason where the per-site kernel runs.  Option 2 takes the tiles only
// in the configuration measured to win.  Known once the planes exist (ones is found with them).
sga::RowSharedTiles tiles(const WindowTraits &t, const char **why);
// Replica groups of a row-shared sweep of window rs_w whose fields kernel is `tiles` (sga_kernels.h, row_shared_groups):
// the count the launch runs.  One wherever the tile plan does not run (the per-site kernels' plan orders its entries across
// all replicas; the sequential windows and every other form have no groups either) and under an energy trace (its stride
// is the call's R).  t.groups = 0: row_shared_default_groups; 1 | 2 | 4: that count, or as many ranges as R gives.  A count
// whose carve of the plan's scratch does not fit is one group.  why: null, or why a count above one was asked for (by the
// caller or the rule) and one group runs.
int groups(const WindowTraits &t, int rs_w, const sga::RowSharedTiles &tiles, bool energy_trace, const char **why);

// ---- the forms' state in an engine, by lifetime -------------------------------------------------------------------------
// Every pointer is device memory the engine allocated; a reset hands what it drops to `release` (the engine: hipFree;
// tests/c_abi/window_state.cpp: a counter) and nulls it.
struct WindowState {
    using Release = void (*)(void *);
    // -- the caller's and the autotuner's own: no reset touches them
    int seq_w = 0;         // sga_set_sequential_windows: W of the sequential windows (0: off), read at every sga_sweep;
                           // not part of sga_export_state
    bool suspend = false;  // true only inside sga_autotune: its geometry trials time the row-per-proposal kernel
    int groups = 0;        // sga_set_replica_groups: 0 the rule's choice, 1 | 2 | 4 forced; not part of sga_export_state
    // -- as long as the engine: the streams and events of the replica groups, made by the first grouped sweep, destroyed
    // by sga_destroy (run.G is set per call)
    sga::RowSharedGroupRun run{};
    // -- per problem: dropped by next_problem() alone; a change of W or of the replicas keeps them
    int grid_planes = 0, grid_k = 0;     // the set-time grid verdict: planes of |2^k J| (0: no verdict) and k; a
                                         // shared-coupling batch: over the batch's words
    unsigned long long *jp = nullptr;    // resident bit-planes of the packed rows (RowSharedPlan::jp), built by the
    int *jabs = nullptr;                 // row-shared form's first sweep of a problem, and sum_j |J_ij| per row
    bool ones = false;                   // found with the planes: every off-diagonal |2^k J_ij| is 1 (sign-only rows)
    bool tiles_refused = false;          // the runtime refused the tile kernel's LDS for this problem
    int8_t *seq_j8 = nullptr;            // resident int8 copy of fp32 rows with |2^k J| <= 127, [n][seq_i8_stride(n)],
    bool seq_j8_refused = false;         // made by the sequential form's first sweep; refused: its allocation failed
    // -- per problem and per replica set: the autotuner's window (0: none) and the rule it was measured under
    int tuned_w = 0, tuned_rule = SGA_RULE_METROPOLIS;
    // -- per replica set: dropped by next_replicas()
    int *seq_base = nullptr;  // [R][seq_base_w] scratch of the sequential windows, made by their first sweep
    int seq_base_w = 0;
    // -- per window plan: the row-shared scratch and what it was sized for; dropped by every reset
    sga::RowSharedPlan rs{};
    int rs_R = 0, rs_n = 0;
    int rs_grid = 0;  // 0 the integer form, else 1 + k (launch_sweep_dense_rs)

    void next_plan(Release release) {
        drop(rs.cnt, release);
        drop(rs.off, release);
        drop(rs.tot, release);
        drop(rs.ent, release);
        drop(rs.base, release);
        drop(rs.bits, release);
        rs = sga::RowSharedPlan{};  // (jp, jabs: views of the problem's)
        rs_R = rs_n = 0;
        rs_grid = 0;
    }
    void next_replicas(Release release) {
        next_plan(release);
        drop(seq_base, release);
        seq_base_w = 0;
        tuned_w = 0;
        tuned_rule = SGA_RULE_METROPOLIS;
    }
    void next_problem(Release release) {  // (the replicas went before: every setter frees them first)
        next_plan(release);
        drop(jp, release);
        drop(jabs, release);
        drop(seq_j8, release);
        seq_j8_refused = false;
        ones = false;
        tiles_refused = false;
        tuned_w = 0;
        tuned_rule = SGA_RULE_METROPOLIS;
        grid_planes = 0;
        grid_k = 0;
    }

private:
    template <typename T>
    static void drop(T *&p, Release release) {
        if (p) release(p);
        p = nullptr;
    }
};

}  // namespace sga_windows

#endif  // SGA_WINDOWS_H
