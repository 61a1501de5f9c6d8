// sga_windows.cpp -- the window forms of the dense sweep (sga_windows.h): the admission rules as pure functions of
// WindowTraits, then -- unless SGA_WINDOWS_PURE is defined, as the stand-alone builds of the tests define it -- the
// engine half: the traits of an engine, the forms' scratch and resident copies, and the plan of one sga_sweep call.
#include "sga_windows.h"

namespace sga_windows {

WindowClass form_class(const WindowTraits &t) {
    WindowClass c;
    if (t.table_m > 0 && !t.acc64) {
        c.planes = sga::row_shared_planes(t.j_abs_max);
        c.jmax = t.j_abs_max;
    } else if (t.row_shared_grid == 1 && t.grid_planes > 0) {
        c.planes = t.grid_planes;
        c.grid = 1 + t.grid_k;
        c.jmax = t.grid_planes <= 3 ? 7 : 255;
    } else {
        c.why = "neither the integer class nor (option row_shared_grid = 1) a grid verdict";
    }
    return c;
}

WindowClass admission(const WindowTraits &t) {
    WindowClass no;
    if (t.rule == SGA_RULE_WOLFF) return (no.why = "the Wolff rule"), no;
    if (t.field_cache != SGA_FIELD_CACHE_OFF) return (no.why = "cached local fields asked for"), no;
    if (!t.dense || t.implicit || t.ragged) return (no.why = "not a dense problem"), no;
    if (t.n_models != 1 && !t.shared_j) return (no.why = "a stacked batch: one matrix per model"), no;
    if (!t.consistent_dE) return (no.why = "J not symmetric with a zero diagonal"), no;
    if (t.force_general != 0) return (no.why = "option force_general"), no;
    if (!t.packed) return (no.why = "no couplings set"), no;
    if ((long long)t.R * t.n >= (1ll << 31)) return (no.why = "R n beyond 2^31 - 1"), no;
    return form_class(t);
}

int row_shared_w(const WindowTraits &t, bool lean) {
    if (t.row_shared == 0 || t.suspend || !lean || t.look_ahead == 0) return 0;
    const WindowClass c = admission(t);
    // (an integer |J| beyond 255 has no bit-planes; the plan's entries keep the replica in 20 bits beside the update)
    if (c.why || c.planes == 0 || t.R >= (1 << 20)) return 0;
    const int tuned = t.rule == t.tuned_rule ? t.tuned_w : 0;  // the autotuner's pick belongs to the rule it timed
    if (t.row_shared == 2) return tuned;
    const long long fw = t.row_shared_window;  // (W for option 1)
    return fw >= 1024 ? 1024 : fw >= 512 ? 512 : fw >= 256 ? 256 : (tuned > 0 ? tuned : 1024);
}

sga::SeqWindows sequential(const WindowTraits &t) {
    // Options "row_shared" and "look_ahead" and the autotuner's suspension do not gate this form (they govern the
    // random-site windows), it has no bound on R alone, and an integer |J| beyond 255 is served (fp32 matrix cores).
    sga::SeqWindows q{};
    if (t.seq_w <= 0 || t.n <= 0) return q;
    const WindowClass c = admission(t);
    if (c.why) return q;
    if (t.want_i8 && c.grid > 1) return q;  // (int8 rows are integers)
    // the product's 16-byte loads walk whole steps of 32 columns: inside the (zero-padded) strides of both operands
    const long long kpad = ((long long)t.n + 31) / 32 * 32;
    if (t.ldj < kpad || (t.R > 0 && (t.sstride % 16 != 0 || t.sstride < kpad))) return q;
    q.grid = c.grid;
    q.mode = (t.want_i8 || c.jmax <= 127) ? 0 : 1;
    q.W = t.seq_w;
    return q;
}

sga::RowSharedTiles tiles(const WindowTraits &t, const char **why) {
    sga::RowSharedTiles s{};
    const char *dummy;
    if (!why) why = &dummy;
    *why = nullptr;
    const int planes = form_class(t).planes;
    if (t.row_shared_fields == 0) return (*why = "option row_shared_fields = 0"), s;
    if (!t.planes_resident) return (*why = "no resident bit-planes"), s;
    if (t.tiles_refused) return (*why = "the tile kernel's LDS request was refused"), s;
    if (t.row_shared_fields == 2 && (*why = sga::row_shared_tiles_not_default(t.n, planes, t.ones))) return s;
    s.S = sga::row_shared_tile_sites(t.n, planes, t.ones, t.R, t.cus, (int)t.row_shared_tile_sites, why);
    s.ones = s.S > 0 && t.ones;
    return s;
}

int groups(const WindowTraits &t, int rs_w, const sga::RowSharedTiles &tiles, bool energy_trace, const char **why) {
    const char *dummy;
    if (!why) why = &dummy;
    *why = nullptr;
    const int asked = t.groups > 0 ? t.groups : sga::row_shared_default_groups(t.R);
    if (asked <= 1) return 1;
    if (rs_w <= 0) return (*why = "not the row-shared windows"), 1;
    if (tiles.S <= 0) return (*why = "the per-site fields kernel: its plan orders the entries across all replicas"), 1;
    if (energy_trace) return (*why = "an energy trace, strided by all replicas"), 1;
    const sga::RowSharedGroups g = sga::row_shared_groups(t.R, asked);
    if (g.G <= 1) return (*why = "32 replicas or fewer"), 1;
    if (!sga::row_shared_groups_fit(t.n, rs_w, tiles.S, t.R, g)) return (*why = "a group's tile plan does not fit its share of the scratch"), 1;
    return g.G;
}

}  // namespace sga_windows

#ifndef SGA_WINDOWS_PURE
#include "sga_engine_impl.h"

namespace sga_impl {

sga_windows::WindowTraits window_traits_of(const sga_engine *e) {
    sga_windows::WindowTraits t;
    t.dense = !e->csr && !e->implicit();
    t.implicit = e->implicit();
    t.ragged = e->ragged;
    t.n_models = e->n_models;
    t.shared_j = e->shared_j;
    t.n = e->n;
    t.R = e->R;
    t.ldj = e->ldj;
    t.sstride = e->sstride;
    t.want_i8 = e->want_i8;
    t.acc64 = e->acc64;
    t.table_m = e->table_m;
    t.j_abs_max = e->j_abs_max;
    t.grid_planes = e->win.grid_planes;
    t.grid_k = e->win.grid_k;
    t.consistent_dE = e->consistent_dE;
    t.packed = e->J_packed != nullptr;
    t.rule = e->rule;
    t.field_cache = e->field_cache;
    t.cus = e->cus;
    t.row_shared = e->opt[OPT_ROW_SHARED];
    t.row_shared_grid = e->opt[OPT_ROW_SHARED_GRID];
    t.row_shared_window = e->opt[OPT_ROW_SHARED_WINDOW];
    t.row_shared_fields = e->opt[OPT_ROW_SHARED_FIELDS];
    t.row_shared_tile_sites = e->opt[OPT_ROW_SHARED_TILE_SITES];
    t.look_ahead = e->opt[OPT_LOOK_AHEAD];
    t.force_general = e->opt[OPT_FORCE_GENERAL];
    t.tuned_w = e->win.tuned_w;
    t.tuned_rule = e->win.tuned_rule;
    t.suspend = e->win.suspend;
    t.seq_w = e->win.seq_w;
    t.planes_resident = e->win.jp != nullptr;
    t.ones = e->win.ones;
    t.tiles_refused = e->win.tiles_refused;
    t.groups = e->win.groups;
    return t;
}

int row_shared_window(const sga_engine *e, bool lean) { return sga_windows::row_shared_w(window_traits_of(e), lean); }
int row_shared_form_planes(const sga_engine *e, int *grid) {
    const sga_windows::WindowClass c = sga_windows::form_class(window_traits_of(e));
    return (*grid = c.grid), c.planes;
}
sga::RowSharedTiles row_shared_tiles(const sga_engine *e, const char **why) { return sga_windows::tiles(window_traits_of(e), why); }
sga::SeqWindows sequential_windows(const sga_engine *e) { return sga_windows::sequential(window_traits_of(e)); }
int replica_groups(const sga_engine *e, int rs_w, const sga::RowSharedTiles &tiles, bool energy_trace, const char **why) {
    return sga_windows::groups(window_traits_of(e), rs_w, tiles, energy_trace, why);
}

// the streams and events of G replica groups: made once, kept as long as the engine; false (and one group runs) if one
// cannot be had
static bool ensure_group_run(sga_engine *e, int G) {
    sga::RowSharedGroupRun &run = e->win.run;
    hipError_t he = hipSuccess;
    if (!run.fork) he = hipEventCreateWithFlags(&run.fork, hipEventDisableTiming);
    for (int g = 0; g + 1 < G && he == hipSuccess; ++g) {
        if (!run.stream[g]) he = hipStreamCreateWithFlags(&run.stream[g], hipStreamNonBlocking);
        if (he == hipSuccess && !run.join[g]) he = hipEventCreateWithFlags(&run.join[g], hipEventDisableTiming);
    }
    if (he != hipSuccess) (void)hipGetLastError();
    return he == hipSuccess;
}

// fp32 rows that the int8 matrix cores can take: their resident int8 copy, made once per problem -- the product reads a
// quarter of the bytes and converts nothing (measured against conversion in registers, DESIGN.md 7: 1.23 -> 0.65 ms of
// product per sweep at n = 10^4, 1024 replicas).  Where the n^2 bytes cannot be had the fp32 matrix cores take the rows
// (exact all the same).
static void ensure_seq_j8(sga_engine *e, sga::SeqWindows &q, hipStream_t st) {
    if (q.mode != 0 || e->want_i8) return;
    sga_windows::WindowState &w = e->win;
    const long long ld8 = sga::seq_i8_stride(e->n);
    if (!w.seq_j8 && !w.seq_j8_refused) {
        hipError_t he = hipMalloc(&w.seq_j8, (size_t)e->n * (size_t)ld8);
        if (he == hipSuccess)
            he = sga::launch_seq_build_i8(static_cast<const float *>(e->J_packed), e->ldj, e->n, q.grid ? q.grid - 1 : 0, w.seq_j8, ld8, st);
        if (he != hipSuccess) {
            (void)hipGetLastError();
            dev_free(w.seq_j8);
            w.seq_j8_refused = true;
        }
    }
    if (!w.seq_j8) {
        q.mode = 1;
        return;
    }
    q.j8 = w.seq_j8;
    q.ld8 = ld8;
}

// its scratch, base[R][W]: made by the form's first sweep, kept until the replicas go; false (and the row-per-proposal
// kernel runs) if it cannot be had
static bool ensure_seq_base(sga_engine *e, int W) {
    sga_windows::WindowState &w = e->win;
    if (w.seq_base && w.seq_base_w >= W) return true;
    dev_free(w.seq_base);
    w.seq_base_w = 0;
    if (hipMalloc(&w.seq_base, sizeof(int) * (size_t)e->R * (size_t)W) != hipSuccess) {
        (void)hipGetLastError();
        w.seq_base = nullptr;
        return false;
    }
    w.seq_base_w = W;
    return true;
}

// the row-shared form's scratch for W and, where the problem gets them, its resident bit-planes of J: false (and the
// row-per-proposal kernel runs) if either cannot be had
static bool ensure_row_shared(sga_engine *e, int W, hipStream_t st) {
    sga_windows::WindowState &w = e->win;
    int grid = 0;
    const int planes = row_shared_form_planes(e, &grid);
    if (w.rs.cnt && w.rs.W == W && w.rs_R == e->R && w.rs_n == e->n && w.rs_grid == grid) return true;
    e->free_row_shared();
    const size_t n = (size_t)e->n, R = (size_t)e->R, nwin = (n + (size_t)W - 1) / (size_t)W;
    const int nw32 = sga::row_shared_nw32(e->n);
    const int log_rg = sga::row_shared_log_group(e->n, W);
    const size_t groups = (R + ((size_t)1 << log_rg) - 1) >> log_rg;
    hipError_t he = hipSuccess;
    if (!w.jp && sga::row_shared_resident(e->want_i8, planes)) {  // once per problem
        he = hipMalloc(&w.jp, sga::row_shared_plane_bytes(e->n, planes));
        if (he == hipSuccess) he = hipMalloc(&w.jabs, sizeof(int) * n);
        if (he == hipSuccess)
            he = sga::launch_rs_build_planes(e->J_packed, e->want_i8, e->ldj, e->n, planes, grid ? grid - 1 : 0, w.jp, w.jabs, st);
        // sign-only rows: one magnitude plane and sum_j |J_ij| = n - 1 in every row -- every off-diagonal |J_ij| (grid
        // form: |2^k J_ij|) is 1, the magnitude plane says nothing the diagonal's place does not (rs_fields_tiles_kernel)
        w.ones = false;
        if (he == hipSuccess && planes == 1) {
            std::vector<int> jabs(n);
            he = hipMemcpyAsync(jabs.data(), w.jabs, sizeof(int) * n, hipMemcpyDeviceToHost, st);
            if (he == hipSuccess) he = hipStreamSynchronize(st);
            w.ones = he == hipSuccess && std::all_of(jabs.begin(), jabs.end(), [&](int v) { return v == (int)n - 1; });
        }
        if (he != hipSuccess) {
            dev_free(w.jp);
            dev_free(w.jabs);
        }
    }
    if (he == hipSuccess) he = hipMalloc(&w.rs.cnt, sizeof(int) * nwin * groups * n);
    if (he == hipSuccess) he = hipMalloc(&w.rs.off, sizeof(int) * nwin * (n + 1));
    if (he == hipSuccess) he = hipMalloc(&w.rs.tot, sizeof(int) * nwin * (size_t)sga::row_shared_scan_chunks(e->n));
    if (he == hipSuccess) he = hipMalloc(&w.rs.ent, sizeof(int) * R * n);
    if (he == hipSuccess) he = hipMalloc(&w.rs.base, sizeof(int) * R * (size_t)W);
    if (he == hipSuccess) he = hipMalloc(&w.rs.bits, sizeof(uint32_t) * R * (size_t)nw32);
    if (he != hipSuccess) {
        (void)hipGetLastError();
        e->free_row_shared();
        return false;
    }
    int lw = 0;
    while ((1 << lw) < W) ++lw;
    w.rs.W = W;
    w.rs.log_w = lw;
    w.rs.nw32 = nw32;
    w.rs.planes = planes;
    w.rs_grid = grid;
    w.rs.jp = w.jp;
    w.rs.jabs = w.jabs;
    w.rs.log_rg = log_rg;
    w.rs.n_groups = (int)groups;
    w.rs_R = e->R;
    w.rs_n = e->n;
    return true;
}

void plan_windows(sga_engine *e, bool lean_call, bool sequential_call, bool energy_trace, int &rs_w, sga::RowSharedTiles &rs_tiles,
                  int &rs_groups, sga::SeqWindows &seq) {
    rs_groups = 1;
    // row-shared windows (sweep_dense_rs.hip): one coupling-row read per proposed site and window
    rs_w = row_shared_window(e, lean_call);
    if (rs_w && !ensure_row_shared(e, rs_w, e->stream)) rs_w = 0;
    if (rs_w) {  // the fields in tiles: the kernel's LDS is asked for here, a refusal leaves the per-site kernel
        rs_tiles = row_shared_tiles(e, nullptr);
        const int planes = e->win.rs.planes;
        // (the tile plan's run starts live in the by-site plan's counts: where they cannot -- many replicas over more
        //  than 32 windows in tiles of a few sites -- the per-site kernel and its plan run)
        if (rs_tiles.S > 0 && sga::row_shared_tile_plan(e->n, rs_w, rs_tiles.S, e->R).rg == 0) rs_tiles = sga::RowSharedTiles{};
        if (rs_tiles.S > 0 &&
            sga::row_shared_tiles_prepare(planes, rs_tiles.ones != 0,
                                          sga::row_shared_tile_lds(e->n, planes, rs_tiles.ones != 0, rs_tiles.S, e->R)) != hipSuccess) {
            (void)hipGetLastError();
            e->win.tiles_refused = true;
            rs_tiles = sga::RowSharedTiles{};
        }
        // replica groups, a stream each (over the tile plan only)
        rs_groups = replica_groups(e, rs_w, rs_tiles, energy_trace, nullptr);
        if (rs_groups > 1 && !ensure_group_run(e, rs_groups)) rs_groups = 1;
    }
    // sequential windows (sweep_dense_seq.hip, sga_set_sequential_windows): one read of each coupling row per sweep
    if (sequential_call) {
        seq = sequential_windows(e);
        if (seq.W && !ensure_seq_base(e, seq.W)) seq.W = 0;
        seq.base = e->win.seq_base;
        if (seq.W) ensure_seq_j8(e, seq, e->stream);
    }
}

}  // namespace sga_impl
#endif  // SGA_WINDOWS_PURE
