// sga_route.cpp -- WHICH kernel form sweeps a problem (sga_route.h).  Everything here is arithmetic on a
// sga_route_query: no device call, no engine state.  The thresholds are measurements (profiles/r0*_experiments.md,
// cited where they stand); tests/test_host_logic.py pins the answers for the five BASELINE configs and the fuzz
// shapes, so an edit that reroutes one of them fails on the CPU.
// (No reference counterpart: the reference has one code path, core/spin_dynamics.py:61-152.)
#include "sga_route.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "sga_kernels.h"
#include "sga_windows.h"

namespace sga_route {

using namespace sga_impl;

namespace {
constexpr long long CSR_TAIL_PAD = 256;       // zeroed entries behind the CSR entry array (sga_engine_impl.h)
constexpr int T2_ELEMS_PER_CHUNK = 8192;      // 1 KiB of one bit-plane
int elems_per_chunk(bool i8) { return i8 ? 1024 : 256; }
bool is_i8(const Query &q) { return q.storage == SGA_J_I8 || q.storage == SGA_J_T2; }
}  // namespace

// ---- set time -------------------------------------------------------------------------------------------------------
// Sparse couplings handed over as a dense matrix (the reference's IsingModel is dense by default; its assignment
// and scheduling encoders fill 1-2 % of it): with SGA_J_AUTO, one model, n >= 4096, integer-valued J and no row of
// more than 256 non-zeros the problem is taken as CSR -- a proposal then reads its row's entries instead of n
// couplings, and the several-updates-per-step forms apply (sweep_csr_rows.hip).  Taken when the caller asked for one
// row read per proposal (field cache OFF), or left the choice (AUTO) on a problem the cached-field sweep cannot
// serve: where that sweep applies it is the better form while few proposals are accepted (C2b, 1024 replicas,
// acceptance 2 %: dense int8 rows 7.7e8, as CSR four updates per step 4.3e9, cached fields 1.06e10 attempts/s).
bool sparse_route_wanted(int storage_requested, int n_models, int n, bool j_integer, int field_cache, bool clf_problem,
                         long long opt_sparse_route) {
    return storage_requested == SGA_J_AUTO && n_models == 1 && n >= 4096 && j_integer &&
           (field_cache == SGA_FIELD_CACHE_OFF || (field_cache == SGA_FIELD_CACHE_AUTO && !clf_problem)) &&
           opt_sparse_route != 0;
}
bool sparse_route_taken(long long longest_row, long long total_entries) {
    return !(longest_row > 256 || total_entries == 0 || total_entries >= (long long)INT32_MAX);
}
// Long rows (mean degree >= 192: the problems that run the wide forms) are padded to whole 64-entry slots.
bool csr_slots_at_set(long long nnz, int n, long long opt_csr_slots) {
    return (double)nnz / std::max(n, 1) >= 192.0 && opt_csr_slots != 0;
}

// ---- dense geometry ---------------------------------------------------------------------------------------------------
// Pick waves-per-replica W and chunks-per-wave CPW for a dense row of C chunks.  Measured on
// MI355X at n = 10^4, R = 1024 (profiles/r01_geometry_sweep.md): full occupancy (R*W ~ 32
// waves per CU) is best as long as every wave keeps >= 4 KiB of the row in flight and W
// balances the four SIMDs; row padding is paid on every read, so it dominates the cost.
bool choose_geometry(int n, int epc, int R, int forced_waves, int &W, int &CPW, int max_cpw, int unit) {
    const int C = (n + epc - 1) / epc;
    // A wave beyond the row's last chunk would hold nothing but pad lanes (every lane redirected
    // to the row's first granule against zero pad spins): a forced count is clamped to the chunk
    // count, so that no geometry the heuristic itself would refuse is reachable by tuning.
    if (forced_waves > C) forced_waves = C;
    double target = 8192.0 / std::max(R, 1);
    target = std::min(16.0, std::max(1.0, target));
    double best_cost = 1e30;
    W = CPW = 0;
    for (int w = 1; w <= sga::MAX_WAVES; ++w) {
        if (forced_waves > 0 && w != forced_waves) continue;
        const int cpw = (C + w - 1) / w;
        if (cpw > max_cpw) continue;
        if (w > C && w > 1) continue;
        const double pad = (double)(w * cpw - C) / C;
        double cost = 4.0 * pad + 0.05 * std::fabs(std::log2(w / target));
        if (cpw * unit < 4 && w > 1) cost += 0.5 * (4 - cpw * unit);   // too little in flight per wave
        if (w > 2 && (w % 4) != 0) cost += 0.03;          // uneven over the 4 SIMDs
        // 9-10 chunks: at the edge of the register file, no look-ahead form (n = 10^4 fp32,
        // 4096 replicas: 4 waves x 10 chunks 1.53e8 attempts/s, 5-16 waves 1.9-2.0e8)
        if (cpw * unit > 8) cost += 0.2;
        if (cost < best_cost) {
            best_cost = cost;
            W = w;
            CPW = cpw;
        }
    }
    if (W == 0) {
        // only reached when the row is too long for the register-resident form (more than max_cpw
        // chunks per wave at the forced / at 16 waves): streaming kernel.  forced_waves <= C here.
        W = forced_waves > 0 ? forced_waves : std::min(sga::MAX_WAVES, C);
        CPW = (C + W - 1) / W;
    }
    return true;
}

long long dense_ldj(const Query &q) {
    if (q.ldj > 0) return q.ldj;
    const long long elem = is_i8(q) ? 1 : 4;
    return ((long long)q.n * elem + 127) / 128 * 128 / elem;
}

// Launch geometry of the dense kernels for the replica count / tuning.  The packed matrices are laid out by n alone
// (at set time), so a change of geometry never touches them.
DenseGeometry dense_geometry(const Query &q) {
    DenseGeometry g;
    const int R = std::max(q.R_local, 1);
    if (q.storage == SGA_J_T2) {
        // bit-plane geometry first; the int8 layout (energy / single-site kernels, non-LEAN sweeps) shares its row
        // length: 8 waves x (Wb * CPWb) chunks of 1024 int8.  At most 4 chunks per wave: a bit-plane chunk costs
        // 8 VGPRs per ring slot
        int Wb, Cb;
        choose_geometry(q.n, T2_ELEMS_PER_CHUNK, R, q.tune_waves, Wb, Cb, sga::T2_MAX_CPW, 1);
        g.ld = (long long)Wb * Cb * T2_ELEMS_PER_CHUNK;
        g.waves = 8;
        g.cpw = Wb * Cb;
        g.waves_t2 = Wb;
        g.cpw_t2 = Cb;
        g.fits = sga::sweep_dense_lds_bytes(g.ld, q.table_m, false) <= 160 * 1024;
    } else if (q.acc == 2) {
        // canonical summation order: a wave owns whole super-chunks of 4 chunks (1024 fp32 elements),
        // one or two of them in registers; longer rows take the streaming form on 16 waves
        int W, S;
        choose_geometry(q.n, 4 * elems_per_chunk(false), R, q.tune_waves, W, S, 2, 4);
        g.waves = W;
        g.cpw = 4 * S;
        g.ld = (long long)W * g.cpw * elems_per_chunk(false);
        g.fits = sga::sweep_dense_lds_bytes(g.ld, q.table_m, true) <= 160 * 1024;
    } else {
        const bool i8 = is_i8(q);
        int W, CPW;
        choose_geometry(q.n, elems_per_chunk(i8), R, q.tune_waves, W, CPW, sga::MAX_CPW, 1);
        g.waves = W;
        g.cpw = CPW;
        g.ld = (long long)W * CPW * elems_per_chunk(i8);
        g.fits = sga::sweep_dense_lds_bytes(g.ld, q.table_m, false) <= 160 * 1024;
    }
    return g;
}

// ---- CSR forms ----------------------------------------------------------------------------------------------------------
// Narrow CSR forms of integer problems whose longest row has <= 64 entries: 0 = one update at a time,
// 1 | 2 = the pair look-ahead (opt-in, option "csr_updates_per_step": round 3 measured -1 ... +3 % on BASELINE configs[2]),
// 4 | 8 = that many updates per step, one per row of 16 | 8 lanes (sweep_csr_rows.hip; the launcher takes it
// for production arguments -- Philox sites, Metropolis with the accept table): the default where it applies
// (profiles/r03_experiments.md 4b: C3, rows of up to 50 entries, 1.0e10 | 2.87e10 | 2.47e10 attempts/s for
// 1 | 4 | 8 updates per step; degree ~16: 1.0e10 | 3.7e10 | 5.1e10).  Option value 0 turns it off.
// Rows of 65 ... 256 entries (assignment / small scheduling problems: degree 100-250, cache resident, bound by the
// one-update chain): four per step with 8 | 16 entries per lane, integer problems with the accept table only.
bool csr_rows_medium(const Query &q) {
    return q.kind == SGA_ROUTE_CSR && q.max_row_len > 64 && q.max_row_len <= 256 && q.acc == sga::CSR_ACC_F32_TABLE &&
           q.table_m > 0;
}
int csr_updates_per_step(const Query &q) {
    if (q.kind != SGA_ROUTE_CSR || q.max_row_len > 256) return 0;
    const bool medium = q.max_row_len > 64;
    if (medium && !csr_rows_medium(q)) return 0;
    int v = q.max_row_len <= 32 ? 8 : 4;
    if (q.opt[OPT_CSR_UPDATES_PER_STEP] >= 0) v = (int)q.opt[OPT_CSR_UPDATES_PER_STEP];
    if (v != 1 && v != 2 && v != 4 && v != 8) return 0;
    if (medium) v = v >= 4 ? 4 : 0;  // (the pair look-ahead holds one wave-load per row)
    if (v >= 4 && (q.layout_entries + CSR_TAIL_PAD) * 8 >= (1ll << 32)) return 0;  // (32-bit byte offsets of the entries)
    return v;
}

CsrForm csr_ragged_form(const Query &q) {
    CsrForm f;
    f.table_m = q.table_m;
    f.sstride = (q.n + 15) / 16 * 16;  // the largest model's spins
    f.waves = 1;
    if (sga::csr_waves_per_block(f.sstride, 0) < 1) f.error = "ragged CSR batch: the largest model does not fit the narrow int8 form";
    else if (q.tune_waves > 1) f.error = "ragged CSR batches run one wave per replica (sga_set_tuning waves_per_replica > 1 picks a wide form)";
    else if (q.opt[OPT_FORCE_CSR_BITS] != 0) f.error = "ragged CSR batches hold int8 spins (option \"force_csr_bits\" picks a bit-spin form)";
    else if (q.opt[OPT_CSR_UPDATES_PER_STEP] > 0)
        f.error = "ragged CSR batches run one update per step (option \"csr_updates_per_step\" > 0 picks another form)";
    else if (q.storage == SGA_CSR_STORAGE_PACKED) f.error = "ragged CSR batches read (column, value) entries (packed storage refused)";
    if (sga::csr_waves_per_block(f.sstride, f.table_m) < 1) f.table_m = 0;  // no room for the table: general path
    return f;
}

// a CSR query with n_models > 1: a ragged batch (sga_set_csr_batch), or one set of rows under n_models field vectors
// (sga_set_csr_shared, shared_j)
static bool csr_ragged(const Query &q) { return q.kind == SGA_ROUTE_CSR && q.n_models > 1 && !q.shared_j; }
static bool csr_shared(const Query &q) { return q.kind == SGA_ROUTE_CSR && q.n_models > 1 && q.shared_j; }

// One set of rows under n_models field vectors: the one-model decision among the one-wave-per-replica forms (int8
// spins, or bit spins with several replicas per workgroup) -- updates per step, medium rows, bits and residency as for
// one model.  The one-replica-per-workgroup forms read a row's h from rowinfo.w, which holds one model's: a problem
// that fits no narrow form, tuning that asks for several waves and packed entries (a wide bit form's) are refused; so are
// cached fields ON (not built for these batches; AUTO streams).  A long-row problem that one model would run wide
// runs narrow here, as a ragged batch does.
CsrForm csr_shared_form(const Query &q) {
    Query one = q;
    one.n_models = 1;
    one.shared_j = 0;
    one.tune_waves = 1;  // (one wave per replica: no wide int8 form, no one-replica-per-workgroup bit form by choice)
    CsrForm f = csr_replica_form(one);
    if (q.tune_waves > 1)
        f.error = "shared-coupling CSR batches run one wave per replica (sga_set_tuning waves_per_replica > 1 picks a "
                  "one-replica-per-workgroup form, whose row records carry one field)";
    else if (q.storage == SGA_CSR_STORAGE_PACKED)
        f.error = "shared-coupling CSR batches read (column, value) entries (packed storage is the one-replica-per-workgroup "
                  "bit form's)";
    else if (q.field_cache == SGA_FIELD_CACHE_ON)
        f.error = "shared-coupling CSR batches: cached local fields are not built for them (SGA_FIELD_CACHE_AUTO runs the "
                  "streaming forms)";
    else if (f.error || f.waves != 1 || f.big_form == 1)
        f.error = "shared-coupling CSR batches: the problem fits no one-wave-per-replica form (int8 spins of a replica beyond "
                  "LDS, and long rows or 64-bit extents rule out the narrow bit form)";
    f.needs_slots = f.wants_packed = false;
    return f;
}

CsrForm csr_replica_form(const Query &q) {
    if (csr_shared(q)) return csr_shared_form(q);
    if (q.n_models > 1) return csr_ragged_form(q);
    CsrForm f;
    const int R_local = q.R_local;
    f.table_m = q.table_m;
    f.sstride = (q.n + 15) / 16 * 16;
    const double deg = (double)q.nnz / q.n;
    const int bits_stride = (q.n + 127) / 128 * 128;
    const bool bits_fit = sga::csr_big_fits(bits_stride, 0);
    // (rows the several-updates-per-step form covers are "short": one wave per replica, several replicas per workgroup)
    // -- while the structure is L2 resident or the replicas are few: beyond that the form is bound by the cache
    // fabric (8-byte entries), where the one-wave bit-spin form with packed 4-byte entries stays ahead (assignment
    // 100 x 100, degree 198, 20 MB: 1024 replicas 1.3e9 -> 3.7e9 attempts/s, 4096 replicas 6.3e9 -> 4.0e9)
    const bool rows_medium = csr_rows_medium(q) && csr_updates_per_step(q) >= 4 && q.tune_waves <= 1 &&
                             (q.layout_entries * 8 <= (6ll << 20) || R_local <= 1024);
    const bool long_rows = deg >= 192.0 && !rows_medium;
    // the bit-spin form that would be used: narrow (several replicas per workgroup, 32-bit
    // extents) on short rows, else one replica per workgroup with its row dealt to waves
    const int rpb_bits = (q.rowptr32 && !long_rows && q.tune_waves <= 1)
                             ? sga::csr_bits_waves_per_block(bits_stride, q.table_m) : 0;
    const bool narrow_bits = rpb_bits >= 2;
    // Spins as bits in LDS: beyond the int8 capacity or the 32-bit extents
    // (option "force_csr_bits": parity tests run the small cases through the same forms) ...
    bool bits = sga::csr_waves_per_block(f.sstride, 0) < 1 || !q.rowptr32 || q.opt[OPT_FORCE_CSR_BITS] != 0;
    // ... or when the int8 spins fit, but not for all replicas at once: workgroups beyond the
    // LDS-resident set run as a second, mostly empty round (C4: 50 KB per replica = 3 per CU
    // = 768 of 1024 replicas resident, 4.7e8 attempts/s; as bits all are resident: 6.8e8)
    if (!bits && bits_fit && q.opt[OPT_CSR_BITS] != 0) {
        const bool wide_i8 = q.tune_waves > 1 || (q.tune_waves == 0 && long_rows && R_local <= 1024);
        const int rpb = wide_i8 ? 1 : std::max(1, sga::csr_waves_per_block(f.sstride, q.table_m));
        const long long budget = 160 * 1024 - 256;
        const long long wg_i8 = (long long)sga::csr_lds_bytes(f.sstride, q.table_m, false) * rpb;
        const long long one_bits = (long long)sga::csr_lds_bytes(bits_stride, q.table_m, true);
        const long long res_i8 = (long long)q.cus * rpb * std::min<long long>(8, budget / wg_i8);
        const long long res_bits =
            narrow_bits ? (long long)q.cus * rpb_bits * std::min<long long>(8, budget / (one_bits * rpb_bits))
                        : (long long)q.cus * std::min<long long>(16, budget / one_bits);
        // Against the one-replica-per-workgroup bit form the barrier-free narrow int8 form with
        // 3-4 replicas per workgroup stays ahead (degree 32, 4096 replicas, n = 40k: 2.35e9 vs
        // 1.77e9 attempts/s with a quarter of the replicas resident; n = 60k, 2 per workgroup:
        // 1.17e9 vs 1.74e9); against the narrow bit form residency decides.
        if (R_local > res_i8 && res_bits > res_i8 && (narrow_bits || wide_i8 || rpb <= 2)) bits = true;
        // (the several-updates-per-step form, sweep_csr_rows.hip, runs on either: 3-D lattice, n = 10 648, 4096
        //  replicas: 3.55e10 attempts/s on int8 spins with 3072 replicas resident, 5.5e10 on bits with all)
    }
    // Long rows with MANY replicas (C5 at 100 cities: degree 396, 2048 replicas): one wave per
    // replica either way, but the slot-addressed bit form (one replica per workgroup, scalar
    // addressing, no per-lane bounds tests) beats the entry-addressed int8 form with four replicas
    // per workgroup: 10.6 vs 11.9 ms per sweep.
    const bool many_long = long_rows && R_local > 1024 && q.tune_waves == 0 && bits_fit && q.slotted &&
                           q.opt[OPT_CSR_BITS] != 0;
    if (many_long) bits = true;
    f.bits = bits;
    f.big_form = !bits ? 0 : (narrow_bits ? 2 : 1);
    if (bits) {
        f.sstride = bits_stride;
        if (!bits_fit) {
            f.error = "CSR problem too large for the LDS-resident spins";
            return f;
        }
        if (!sga::csr_big_fits(f.sstride, f.table_m)) f.table_m = 0;
        if (f.big_form == 2) {
            f.waves = 1;
        } else {
            // one workgroup per replica: deal a long row to as many waves as the 8 entries per
            // lane requested ahead need to cover it (profiles/r01_experiments.md: 500 cities,
            // degree 1996: 4 waves; 1000 cities, 3996: 8)
            const int wpr = q.tune_waves > 0 ? q.tune_waves : (many_long ? 1 : (int)std::ceil(deg / 512.0));
            f.waves = std::max(1, std::min(wpr, 8));
        }
    } else {
        if (sga::csr_waves_per_block(f.sstride, f.table_m) < 1)
            f.table_m = 0;  // no room for the probability table: general path
        // Long rows AND too few replicas to give every SIMD a wave: deal each row to two waves
        // (one replica per workgroup).  The kernel is issue bound, so with >= 2048 replicas the
        // extra waves only repeat the per-update work (measured: C4, R = 1024: 1 / 2 / 4 / 8
        // waves -> 2.98 / 3.69 / 3.67 / 3.34 e8 attempts/s; C5, R = 2048: 1.55 vs 1.19 e9).
        const int wpr = q.tune_waves > 0 ? q.tune_waves : ((long_rows && R_local <= 1024) ? 2 : 1);
        f.waves = std::min(wpr, 8);
    }
    // the wide builds exist for 1, 2, 4 and 8 waves per replica (slot arithmetic on constants; the
    // canonical summation order of real-valued rows is defined on that grid)
    {
        int p2 = 1;
        while (p2 < f.waves) p2 *= 2;
        f.waves = std::min(p2, 8);
    }
    // one replica per workgroup (row dealt to its waves): rows are addressed by 64-entry slots
    f.needs_slots = f.waves > 1 || f.big_form == 1;
    f.wants_packed = f.big_form == 1 && q.storage != SGA_CSR_STORAGE_F32;
    return f;
}

int csr_replicas_per_block(const Query &q, const CsrForm &f) {
    (void)q;
    return f.big_form == 2 ? sga::csr_bits_waves_per_block(f.sstride, f.table_m)
                           : ((f.waves > 1 || f.bits) ? 1 : sga::csr_waves_per_block(f.sstride, f.table_m));
}

const char *csr_kernel_family(const Query &q, const CsrForm &f, bool slotted_now) {
    // the order of launch_sweep_csr (sweep_csr.hip) for production arguments: Philox sites, Metropolis, fp64, no traces
    sga::SweepArgs a{};
    a.rowptr = q.rowptr32 ? reinterpret_cast<const int32_t *>(8) : nullptr;  // (only tested against null)
    a.big = f.big_form;
    a.csr_row_cap = (q.max_row_len <= 256) ? (int)std::max<long long>(slotted_now ? (q.max_row_len + 63) / 64 * 64 : q.max_row_len, 1) : 0;
    a.csr_pair_ahead = csr_updates_per_step(q);
    a.csr_acc = q.acc;
    a.table_m = f.table_m;
    if (a.csr_acc == sga::CSR_ACC_F32_TABLE && a.table_m == 0) a.csr_acc = sga::CSR_ACC_F32;
    a.table_scale = q.table_scale > 0 ? q.table_scale : 1;
    a.site_mode = SGA_SITE_RANDOM;
    a.arith = SGA_ARITH_F64;
    a.rule = SGA_RULE_METROPOLIS;
    a.look_ahead = q.opt[OPT_LOOK_AHEAD] != 0 ? 1 : 0;
    a.force_general = q.opt[OPT_FORCE_GENERAL] != 0 ? 1 : 0;
    a.sstride = f.sstride;
    if (f.waves == 1 && sga::sweep_csr_rows_applies(a)) return "rows";
    if (f.bits) return (f.waves == 1 && q.rowptr32 && f.big_form == 2) ? "narrow-bits" : "wide-bits";
    return f.waves > 1 ? "wide-bytes" : "narrow";
}

// ---- TSP-structured couplings --------------------------------------------------------------------------------------------
// 256 cities per wave and pass.  Four or more waves at one pass: half the waves with two passes each do better (1000
// cities, same box: 4 x 1 711 ms, 2 x 2 677 ms, 1 x 4 701 ms per sweep -- fewer barrier participants against a longer
// row sum); tuning may ask otherwise.
TspForm tsp_form(int npad, int tune_waves) {
    TspForm t;
    const int full = npad / 256;  // waves at one pass
    int w = (full >= 4 && full % 2 == 0) ? full / 2 : full;
    if (tune_waves == full) w = full;
    if (tune_waves > 0 && tune_waves < full && full % tune_waves == 0 && (full / tune_waves == 2 || full / tune_waves == 4))
        w = tune_waves;
    t.waves = w;
    t.passes = full / w;
    return t;
}

// ---- couplings as a sum of complete graphs on groups ---------------------------------------------------------------------
// One wave decides 128 proposals per round, and a round costs the same whatever the number of waves beside it, so a
// replica gets as many waves as leave every CU its share of replicas at four waves per SIMD (16 per CU): 1024 replicas
// on 256 CUs = 4 waves each.  Tuning (sga_set_tuning waves_per_replica = 1 | 2 | 4 | 8) overrides.
GroupsForm groups_form(const Query &q) {
    GroupsForm f;
    f.sstride = (int)(((long long)q.n + 127) / 128 * 128);
    f.wide = q.group_max >= (1 << 15);
    f.lds_bytes = std::max(sga::groups_lds_bytes(f.sstride, std::max(q.n_groups, 1), f.wide ? 1 : 0),
                           sga::groups_energy_lds_bytes(f.sstride, std::max(q.n_groups, 1), f.wide ? 1 : 0));
    if (f.lds_bytes > 160 * 1024 - 256) f.error = "spin bits and group sums of a replica do not fit LDS (160 KiB)";
    const long long windows = ((long long)q.n + 127) / 128;  // 128 proposals per wave and round
    const int per_cu = (std::max(q.R_local, 1) + std::max(q.cus, 1) - 1) / std::max(q.cus, 1);
    int w = 16 / std::max(per_cu, 1);
    w = w >= 8 ? 8 : w >= 4 ? 4 : w >= 2 ? 2 : 1;
    while (w > 1 && w > windows) w >>= 1;
    if (q.tune_waves == 1 || q.tune_waves == 2 || q.tune_waves == 4 || q.tune_waves == 8) w = q.tune_waves;
    f.waves = w;
    return f;
}

// ---- cached local fields ----------------------------------------------------------------------------------------------------
// A dense query under option "clf_fixed_point" = 1 whose problem the integer form does not take (clf_ok = 0) carries the
// fixed-point form in clf_bits: 32 | 64 = the width of its fields, 0 = the set-time scan refused it (acc = 2: the
// f64-canonical class).  clf_ok = 1 keeps clf_bits = 16 | 32 of the integer form.
bool dense_fixed_point(const Query &q) {
    return q.kind == SGA_ROUTE_DENSE && q.opt[OPT_CLF_FIXED_POINT] == 1 && !q.clf_ok && (q.clf_bits == 32 || q.clf_bits == 64);
}
// The cached-local-field sweep serves: dense integer-valued symmetric problems (one model, or a many-model batch that
// qualifies over all its stacked rows) whose fields and spin bits fit LDS, and CSR problems with integer J in strictly sorted rows -- any single-site rule.
const char *clf_refusal(const Query &q) {
    if (q.kind == SGA_ROUTE_TSP) return "cached local fields: stored couplings only";
    if (q.kind == SGA_ROUTE_GROUPS)
        return "cached local fields: stored couplings only (sga_set_groups keeps the group sums resident instead; AUTO runs "
               "that form as it is)";
    if (csr_shared(q))
        return "shared-coupling CSR batches: cached local fields are not built for them (SGA_FIELD_CACHE_AUTO runs the "
               "streaming forms)";
    if (csr_ragged(q) && q.opt[OPT_RAGGED_FIELD_CACHE] == 0)
        return "cached local fields: not built for ragged CSR batches (sga_set_csr_batch runs the streaming narrow form)";
    if (csr_ragged(q)) {
        // option "ragged_field_cache": the int16 form of sweep_clf_csr.hip, each replica on its own model's rows; LDS is
        // laid out for the largest model (q.n), the table and the longest row are the batch's
        const long long ldf = ((long long)q.n + 127) / 128 * 128;
        if (q.opt[OPT_CLF_FIXED_POINT] == 1 && (q.clf_bits == 32 || q.clf_bits == 64)) {
            // ... with option "clf_fixed_point": a batch the int16 form does not take, D = 2^k J_m s as exact int32 | int64
            // with one k and one width for the batch, no accept table
            if (!q.clf_ok || q.acc == sga::CSR_ACC_F64_CANON)
                return "cached local fields over ragged CSR batches (fixed point) need, in every model, acc class f32 / f64-exact, "
                       "strictly sorted rows (no duplicates), and 2^k max_i sum_j |J_ij| < 2^53 at the batch-wide k";
            if (q.max_row_len > 4 * 64 * 8)
                return "cached local fields over ragged CSR batches (fixed point): a row is longer than 2048 entries";
            if (q.R_local > 0 && sga::sweep_clf_csr_lds_bytes(ldf, q.sstride, 0, q.clf_bits) > 160 * 1024)
                return q.clf_bits == 64 ? "cached local fields over ragged CSR batches (fixed point): int64 fields and spins of the "
                                          "largest model do not fit LDS (160 KiB: n_max <= ~20 000)"
                                        : "cached local fields over ragged CSR batches (fixed point): int32 fields and spins of the "
                                          "largest model do not fit LDS (160 KiB: n_max <= ~39 000)";
            return nullptr;
        }
        if (!q.clf_ok)
            return "cached local fields over ragged CSR batches need, in every model, integer-valued J in strictly sorted rows "
                   "(no duplicates), h in multiples of 1/2, max_i sum_j |J_ij| < 2^15 and the accept table";
        if (q.max_row_len > 4 * 64 * 8) return "cached local fields over ragged CSR batches: a row is longer than 2048 entries";
        if (q.R_local > 0 && (q.table_m <= 0 || sga::sweep_clf_csr_lds_bytes(ldf, q.sstride, q.table_m) > 160 * 1024))
            return "cached local fields over ragged CSR batches: fields, spins and accept table of the largest model do not "
                   "fit LDS (160 KiB)";
        return nullptr;
    }
    if (q.kind == SGA_ROUTE_CSR) {
        // sparse couplings: the dynamic part of the fields as int16 in LDS (sweep_clf_csr.hip)
        const long long ldf = ((long long)q.n + 127) / 128 * 128;
        if (!q.clf_ok)
            return q.from_dense
                       ? "cached local fields: this sparse matrix was kept as CSR because the field cache was OFF when "
                         "sga_set_dense ran (its dense source is released), and as CSR it does not qualify (integer J in "
                         "strictly sorted rows, sum_j |J_ij| < 2^15, h in multiples of 1/2) -- call sga_set_field_cache "
                         "before sga_set_dense"
                       : "cached local fields over CSR couplings need integer-valued symmetric J in strictly sorted rows "
                         "(no duplicates), zero diagonal, max_i sum_j |J_ij| < 2^15 and h in multiples of 1/2";
        if (q.opt[OPT_CLF_FIXED_POINT] == 1 && (q.clf_bits == 32 || q.clf_bits == 64)) {
            // option "clf_fixed_point": D = 2^k J s as exact int32 | int64 (sweep_clf_csr.hip), no accept table
            if (!q.clf_ok)
                return q.acc == sga::CSR_ACC_F64_CANON
                           ? "cached local fields (fixed point): acc class f64-canonical -- no exact fixed point holds a row sum"
                           : "cached local fields (fixed point): need symmetric J in strictly sorted rows (no duplicates) "
                             "and a zero diagonal";
            if ((q.slotted ? (q.max_row_len + 63) / 64 * 64 : q.max_row_len) > 4 * 64 * 8)
                return q.clf_bits == 64 ? "cached local fields (fixed point, int64 fields): a row is longer than 2048 entries"
                                        : "cached local fields (fixed point, int32 fields): a row is longer than 2048 entries";
            if (q.R_local > 0 && sga::sweep_clf_csr_lds_bytes(ldf, q.sstride, 0, q.clf_bits) > 160 * 1024)
                return q.clf_bits == 64 ? "cached local fields (fixed point): int64 fields and spins of a replica do not fit "
                                          "LDS (160 KiB: n <= ~20 000)"
                                        : "cached local fields (fixed point): int32 fields and spins of a replica do not fit "
                                          "LDS (160 KiB: n <= ~40 000)";
            return nullptr;
        }
        if (q.opt[OPT_CLF_FIXED_POINT] == 1 && !q.clf_ok && q.acc == sga::CSR_ACC_F64_CANON)
            return "cached local fields (fixed point): acc class f64-canonical -- no exact fixed point holds a row sum";
        if (q.R_local > 0 && (sga::sweep_clf_csr_lds_bytes(ldf, q.sstride, q.table_m) > 160 * 1024 ||
                              (q.slotted ? (q.max_row_len + 63) / 64 * 64 : q.max_row_len) > 4 * 64 * 8))
            return "cached local fields: fields and spins of a replica do not fit LDS (or a row is longer than 2048 entries)";
        return nullptr;
    }
    if (!q.clf_ok && dense_fixed_point(q)) {
        // option "clf_fixed_point": D = 2^k J s as exact int32 | int64 (sweep_clf_fx.hip), no accept table
        if (q.R_local > 0 && sga::sweep_clf_fx_lds_bytes((dense_ldj(q) + 127) / 128 * 128, q.clf_bits, q.sstride) > 160 * 1024)
            return q.clf_bits == 64 ? "cached local fields (fixed point): int64 fields and spins of a replica do not fit "
                                      "LDS (160 KiB: n <= ~20 000)"
                                    : "cached local fields (fixed point): int32 fields and spins of a replica do not fit "
                                      "LDS (160 KiB: n <= ~39 000)";
        return nullptr;
    }
    if (!q.clf_ok && q.opt[OPT_CLF_FIXED_POINT] == 1 && q.clf_bits == 0) {
        // (the set-time scan refused the fixed-point form; the engine reports its own, more precise reason)
        // (many-model batches: only under option "batch_fixed_point", set with "clf_fixed_point" before sga_set_dense_batch)
        if (q.n_models > 1 && q.opt[OPT_BATCH_FIXED_POINT] == 0)
            return "cached local fields (fixed point): not built for dense batches (one model only)";
        if (q.acc == 2)
            return "cached local fields (fixed point): acc class f64-canonical -- no exact fixed point holds a row sum";
        return "cached local fields (fixed point): need symmetric J with a zero diagonal and fields within int64";
    }
    if (!q.clf_ok)
        return "cached local fields need integer-valued symmetric J with a zero diagonal, h in multiples of 1/2 and row "
               "sums below 2^24 (a dense batch: in every model)";
    if (q.R_local > 0 && sga::sweep_clf_lds_bytes((dense_ldj(q) + 127) / 128 * 128, q.clf_bits, q.sstride,
                                                  q.clf_scale == 2 ? 2048 : q.table_m) > 160 * 1024)
        return "cached local fields: fields and spins of a replica do not fit LDS";
    return nullptr;
}

// Break-even acceptance of ONE replica = (what an update costs its chain on the row kernel) / (what an accept costs it
// on the cached-field kernel).  Both kernels are paced by a replica's serial chain, not by the chip, whenever only
// part of the replicas is hot: ~1.5 us per accept (1.15 alone on its CU ... 1.7 with busy neighbours), and per update
// 0.38 us on bit-planes / 0.58 us on int8 rows at n = 10^4, ~0.3 us on short rows (profiles/r04_routing.py; fp32
// rows: estimate).
// Option "clf_fixed_point": the fixed-point cached-field sweep has no accept table -- every proposal of a window takes
// the exp path -- and moves 4 | 8-byte fields.  The cost per accept in the units of t_upd is set from the measured
// break-even (profiles/fixed_point_fields.json): C5 at 100 cities (int64), 2.0 against 8.6 ms per sweep at 0.38 %
// acceptance -- ~1.5 ms of windows plus ~1.5 us per accept: break-even near 6 % --, and a 20 000-spin binary-grid
// instance (int32), 18.4 against 3.96 ms at 15.9 %: near 3.4 %.
// Ragged batches under "ragged_field_cache" too: the same two costs per accept, against the hottest replica's acceptance
// over its own n_m -- NOT measured for ragged batches as a break-even (profiles/ragged_fixed_point.json reports whole
// windows of an SA run).
static double fixed_point_theta(const Query &q, double t_upd) {
    const double t_acc = q.clf_bits == 64 ? 8.8 : 6.3;
    return t_upd / t_acc;
}
// Dense fixed point (sweep_clf_fx.hip): no accept table either, and an accept scales every entry of its row in fp64
// before it moves the 4 | 8-byte fields.  The cost per accept, in the units of t_upd below, from
// profiles/dense_fixed_point.json (binary-grid SK, n = 10^4, int32, 1024 replicas): on a ladder that stays hot (1000 ->
// 20, hottest replica 92 % acceptance) the launch is that replica's chain, 42.6 ms for 9 213 accepts = 4.6 us per accept,
// against 54.0 ms / 10^4 = 5.4 us per update on the fp32 row kernel: an accept costs 0.86 updates, t_acc = 0.86 x t_upd
// (n = 10^4: 1.5) = 1.3 -- a replica at n = 10^4 is never given to the row kernels (theta 1.15; every measured line,
// 0.2 % to 47 % mean acceptance, is faster cached: 1.1 - 1.3 ms against 54 ms per sweep at 1 %).  int64: not measured at
// size; 1.5 by the field bytes an accept moves (estimate).
// Many-model batches (option "batch_fixed_point"): the same two figures -- NOT measured for batches as a break-even (a
// batch has few replicas per model and a mostly empty chip; profiles/batch_fixed_point.json reports whole runs).
constexpr double DENSE_FX_T_ACC32 = 1.3, DENSE_FX_T_ACC64 = 1.5;
static double dense_fixed_point_theta(const Query &q, double t_upd) {
    const double t_acc = q.clf_bits == 64 ? DENSE_FX_T_ACC64 : DENSE_FX_T_ACC32;
    return t_upd / t_acc;
}
double routing_theta(const Query &q) {
    const double kn = (double)q.n / 1000.0;
    // (ragged batches: q.n is the largest model, so nnz / n overstates the mean row; no row is longer than the longest)
    const double deg = csr_ragged(q) ? std::min((double)q.nnz / (double)q.n, (double)q.max_row_len)
                                                                     : (double)q.nnz / (double)q.n;
    const double t_upd = q.kind == SGA_ROUTE_CSR ? 0.20 + 0.0008 * deg  // (C4: 0.68, C2b as CSR: 0.36)
                         : q.storage == SGA_J_T2 ? 0.29 + 0.009 * kn
                                                 : (q.storage == SGA_J_I8 ? 0.27 + 0.031 * kn : 0.30 + 0.12 * kn);
    if (q.kind == SGA_ROUTE_CSR && q.opt[OPT_CLF_FIXED_POINT] == 1 && (q.clf_bits == 32 || q.clf_bits == 64))
        return fixed_point_theta(q, t_upd);
    if (dense_fixed_point(q)) return dense_fixed_point_theta(q, t_upd);
    return t_upd / 1.5;
}
// AUTO, nothing known yet: the run starts on the kernel that loses least if the guess is wrong: the cached-field
// kernel where a replica would have to accept more than ~30 % of its proposals for the row kernels to win (int8 and
// fp32 rows at n = 10^4: the first four sweeps of the bench ladder 55 / 218 ms on the row kernels against 8 / 30 ms
// cached, and 36 against 56 / 208 ms on a ladder that stays hot), the row-per-proposal kernel otherwise (bit-planes,
// small n, CSR).
// Many-model dense batches start cached from n = 1024 on: a batch has few replicas per model, the chip is mostly empty
// and the run is paced by each replica's serial chain, where the cached kernel is ahead from the first sweep -- sweeps
// 0..10 of the default SA schedule from random spins, 32 models x 1 replica, int8 rows: 0.128 against 0.288 ms per
// sweep at n = 1024 (11 % acceptance), 0.39 / 1.32 at 4096, 0.93 / 4.94 at 10^4; behind at n = 256 (0.246 / 0.209, 19 %)
// and n = 128 (0.076 / 0.058, 27 %) -- profiles/batch_cached_fields.json.  The thresholds after the start are the
// one-model ones.
bool auto_starts_cached(const Query &q) {
    if (q.kind == SGA_ROUTE_DENSE && q.n_models > 1) return q.n >= 1024 || 0.8 * routing_theta(q) >= 0.3;
    return q.kind != SGA_ROUTE_CSR && 0.8 * routing_theta(q) >= 0.3;
}

int clf_csr_waves(const Query &q) {
    const long long row_max = std::min<long long>(q.slotted ? (q.max_row_len + 63) / 64 * 64 : q.max_row_len, 1 << 20);
    return (row_max > 256 || q.n > 20000) ? 8 : 4;
}

// sweeps per launch: aim for ~50 ms of estimated work per launch
int sweeps_per_launch(const Query &q, int n_sweeps, int tune_spl, int npad_tsp) {
    int spl = tune_spl;
    if (spl <= 0) {
        const double row_bytes = q.kind == SGA_ROUTE_GROUPS ? 64.0  // (no row: a few table entries per proposal)
                                 : q.kind == SGA_ROUTE_TSP ? 8.0 * npad_tsp
                                 : q.kind == SGA_ROUTE_CSR ? 264.0 : (double)dense_ldj(q) * (is_i8(q) ? 1 : 4);
        const double per_update = std::max(row_bytes * q.R_local / 4.0e12, 1.0e-6);
        const double per_sweep = per_update * q.n;
        spl = (int)std::min<double>(n_sweeps, std::max(1.0, std::floor(0.05 / per_sweep)));
    }
    return std::max(1, std::min(spl, n_sweeps));
}

// ---- the cached-field modes' look at the acceptance counters -------------------------------------------------------------
// AUTO routes every replica by ITS OWN acceptance: the cached-field kernel costs a replica ~1.1 - 1.7 us of its
// serial chain per ACCEPTED proposal and next to nothing per rejected one, the row-per-proposal kernels cost
// every replica the same per update whatever happens (~0.4 us on bit-planes, ~1.3 us on int8 rows, ~5 us on
// fp32 rows at n = 10^4) -- so a replica belongs on the row kernels only while its acceptance exceeds the ratio
// of the two (profiles/r04_experiments.md 2), and a ladder with a hot end runs as TWO concurrent launches (two
// streams) over disjoint replica lists.  The chain of a replica does not depend on the kernel that walks it.
// The per-replica counters are read back every 4 ... 16 sweeps.  Without per-replica routing (option
// "replica_routing" = 0; CSR couplings, whose row kernels take no replica lists): one launch, decided by the hottest
// replica.
// Both cached-field modes (ON and AUTO) look at the per-replica acceptance now and then.  A launch of the cached-field
// kernel ends with its hottest replica's serial chain; once most replicas accept next to nothing -- their workgroups
// are gone early and the chip idles behind that one chain -- EVERY replica gets eight waves (option "clf_tail_waves"):
// the workgroups then run as two rounds, which costs where the replicas are busy (sweeps 5-25 of the 10 000-spin ladder:
// 0.42 against 0.27 ms per sweep) and pays in the tail (after 100 sweeps 0.098 against 0.106;
// profiles/r04_experiments.md 9).  Giving only the hottest replicas eight waves in a launch of their own did not:
// beside the four-wave workgroups of the others their rounds took 1.6 us instead of 0.9.
// Option "clf_batched" = 2 (default): the form that commits several accepts per round (sweep_clfb_impl.h) while the
// hottest replica accepts more than ~1 % of its proposals -- 16 % ahead on the first sweeps from random spins, 10 %
// at sweeps 5-25 of the 10 000-spin ladder -- and one accept per round below (7 % ahead after 100 sweeps).
ClfLooks clf_looks(const Query &q, bool sized) {
    ClfLooks l;
    const bool dense = q.kind != SGA_ROUTE_CSR;
    l.is_auto = q.field_cache == SGA_FIELD_CACHE_AUTO;
    l.tail = dense && q.opt[OPT_CLF_TAIL_WAVES] != 0 && q.opt[OPT_CLF_WAVES] == 0 &&
             (!sized || (sga::sweep_clf_waves(q.ldj, is_i8(q), q.R_local, q.cus, (int)q.opt[OPT_CLF_WAVES]) < 8 &&
                         q.ldj >= 6 * elems_per_chunk(is_i8(q)) && q.R_local >= 16));
    l.adaptive = dense && q.opt[OPT_CLF_BATCHED] == 2;
    return l;
}

bool look(ReplicaRouting &s, const LookInput &in, const std::function<const unsigned long long *()> &read_counters) {
    const size_t R = (size_t)in.R;
    if (s.mark_acc.size() != R) {  // nothing known yet: a run starts hot, four sweeps to the first look
        s.reset();
        s.mark_acc.assign(R, 0ull);
        s.route.assign(R, in.start_cached ? 0 : 1);
        s.n_cached = in.start_cached ? in.R : 0;
    }
    const long long since = in.attempted - s.mark_attempted;
    if (since >= 0 && since < (long long)s.interval * in.n) return false;
    const unsigned long long *now = read_counters();
    if (!now) return false;
    bool back = false;
    auto accepts = [&](size_t r) { return now[r] - s.mark_acc[r]; };
    if (since > 0) {
        if (in.looks.is_auto) {
            // (enter, leave): acceptance below which a replica is taken onto the cached-field kernel, above which it is
            // given back (hysteresis).  Break-even acceptance of ONE replica (theta: routing_theta) = (what an update
            // costs its chain on the row kernel) / (what an accept costs it on the cached-field kernel).  Both kernels
            // are paced by a replica's serial chain, not by the chip, whenever only part of the replicas is hot: ~1.5 us
            // per accept (1.15 alone on its CU ... 1.7 with busy neighbours), and per update 0.38 us on bit-planes /
            // 0.58 us on int8 rows at n = 10^4, ~0.3 us on short rows (profiles/r04_routing.py; fp32 rows: estimate).
            const double enter = 0.8 * in.theta, leave = 1.2 * in.theta;
            if (in.per_replica) {
                for (size_t r = 0; r < R; ++r) {
                    const double acc = (double)accepts(r) / (double)since;
                    int &rt = s.route[r];
                    if (rt == 0 && acc > leave) rt = 1;
                    else if (rt == 1 && acc < enter) rt = 0, back = true;
                }
            } else {
                // (ragged batches: `since` counts n_max attempts per sweep, replica r made n_m of them)
                double hottest = 0.0;
                for (size_t r = 0; r < R; ++r)
                    hottest = std::max(hottest, (double)accepts(r) / ((double)since * (double)(in.spins ? in.spins[r] : in.n) /
                                                                     (double)in.n));
                const bool was = s.n_cached > 0;
                const bool use = was ? hottest < leave : hottest < enter;
                back = use && !was;
                s.route.assign(R, use ? 0 : 1);
            }
        }
        // the replicas on the cached-field kernel: how many, the hottest one's accepts, and the sum in accepts per sweep
        const double per_sweep = (double)in.n / (double)since;  // counter difference -> accepts per sweep
        unsigned long long top = 0;
        double asum = 0.0;
        int cnt = 0;
        for (size_t r = 0; r < R; ++r) {
            if (s.route[r] != 0) continue;
            ++cnt;
            top = std::max(top, accepts(r));
            asum += (double)accepts(r) * per_sweep;
        }
        s.n_cached = cnt;
        // (hysteresis: in above 1.5 % of the hottest replica's proposals, out below 1 %)
        if (in.looks.adaptive && cnt > 0) s.hot = (double)top / (double)since > (s.hot ? 0.010 : 0.015);
        // (mean / hottest ~ the share of the launch during which the chip is busy: measured ahead at 0.21,
        //  behind at 0.38 -- in below 0.28, out above 0.36; a chain of two dozen accepts per sweep is the
        //  least that matters against the windows of a sweep)
        const double amax = (double)top * per_sweep;
        s.wide = in.looks.tail && cnt > 0 && !(in.looks.adaptive && s.hot) && amax >= 24.0 &&
                 asum / (double)cnt / std::max(amax, 1.0) < (s.wide ? 0.36 : 0.28);
        s.interval = std::min(16, s.interval * 2);
        s.dirty = true;
    }
    s.mark_acc.assign(now, now + R);
    s.mark_attempted = in.attempted;
    return back;
}

// ---- the window forms' admission rules over a query (sga_windows.h) ------------------------------------------------------
sga_windows::WindowTraits window_traits_of_query(const Query &q) {
    sga_windows::WindowTraits t;
    t.dense = q.kind == SGA_ROUTE_DENSE;
    t.n_models = q.n_models;
    t.shared_j = q.shared_j != 0;
    t.n = q.n;
    t.ldj = q.ldj;
    t.sstride = q.sstride;
    t.want_i8 = is_i8(q);
    t.acc64 = q.acc != 0 && !t.want_i8;  // (int8 rows sum in int32 whatever q.acc says)
    t.table_m = q.table_m;
    t.grid_planes = q.rs_grid > 0 ? 1 : 0;  // assumed: a query carries k alone -- some verdict, the fewest planes
    t.grid_k = q.rs_grid > 0 ? q.rs_grid - 1 : 0;
    t.field_cache = q.field_cache;
    t.cus = q.cus;
    t.row_shared = q.opt[sga_impl::OPT_ROW_SHARED];
    t.row_shared_grid = q.opt[sga_impl::OPT_ROW_SHARED_GRID];
    t.row_shared_fields = q.opt[sga_impl::OPT_ROW_SHARED_FIELDS];
    t.row_shared_tile_sites = q.opt[sga_impl::OPT_ROW_SHARED_TILE_SITES];
    t.look_ahead = q.opt[sga_impl::OPT_LOOK_AHEAD];
    t.force_general = q.opt[sga_impl::OPT_FORCE_GENERAL];
    t.consistent_dE = q.clf_ok != 0;  // assumed: the cached-field verdict stands in for "symmetric, zero diagonal"
    t.j_abs_max = 1;                  // assumed: |J| within the planes' range (a query carries no maximum)
    t.R = 0;                          // assumed: the replica bounds are met (R n < 2^31, R < 2^20)
    t.packed = true;                  // assumed: the couplings are set
    t.rule = SGA_RULE_METROPOLIS;     // assumed: a query carries no rule
    t.row_shared_window = 0;          // assumed: the default window -- with no tuned pick (tuned_w = 0), option 1 gives
                                      // W = 1024 and option 2 no window
    return t;
}

// ---- the whole chain of decisions as one line ----------------------------------------------------------------------------
std::string explain(const Query &q0) {
    Query q = q0;
    char buf[640];
    std::string out;
    if (q.kind == SGA_ROUTE_GROUPS) {
        const GroupsForm f = groups_form(q);
        if (f.error) return std::string("groups error=") + f.error;
        const bool general = q.opt[OPT_FORCE_GENERAL] != 0;
        std::snprintf(buf, sizeof(buf), "groups n_groups=%d largest_group=%d sums=%s waves=%d sstride=%d lds_bytes=%zu kernel=%s",
                      q.n_groups, q.group_max, f.wide ? "int32" : "int16", general ? 1 : f.waves, f.sstride, f.lds_bytes,
                      general ? "sweep_groups_general_kernel" : "sweep_groups_kernel|sweep_groups_general_kernel");
        out = buf;
        if (q.rest_nnz > 0) {  // sga_set_groups_csr: the stored remainder
            std::snprintf(buf, sizeof(buf), " rest_nnz=%lld rest_max_row=%d", (long long)q.rest_nnz, q.rest_max_row);
            out += buf;
        }
        q.sstride = f.sstride;
    } else if (q.kind == SGA_ROUTE_TSP) {
        const int npad = 256 * ((q.n_cities + 255) / 256);
        const TspForm t = tsp_form(npad, q.tune_waves);
        std::snprintf(buf, sizeof(buf), "tsp n_cities=%d waves=%d passes=%d updates_per_step_option=%lld kernel=%s", q.n_cities,
                      t.waves, t.passes, (long long)q.opt[OPT_TSP_PARALLEL],
                      q.opt[OPT_TSP_PARALLEL] == 0 ? "sweep_tsp_kernel" : "sweep_tsp_par_kernel|sweep_tsp_kernel");
        out = buf;
    } else if (csr_ragged(q)) {
        const CsrForm f = csr_ragged_form(q);
        if (f.error) return std::string("csr error=") + f.error;
        std::snprintf(buf, sizeof(buf),
                      "csr form=narrow ragged models=%d spins=int8 waves=1 replicas_per_block=%d updates_per_step=1 slots=0 "
                      "entries=cv table_m=%d sstride=%d",
                      q.n_models, sga::csr_waves_per_block(f.sstride, f.table_m), f.table_m, f.sstride);
        out = buf;
        q.sstride = f.sstride;
    } else if (q.kind == SGA_ROUTE_CSR) {
        const CsrForm f = csr_replica_form(q);
        if (f.error) return std::string("csr error=") + f.error;
        const bool slotted_now = q.slotted || f.needs_slots;
        if (slotted_now && !q.slotted) {  // ensure_slotted re-pads the layout: at most 63 entries more per row
            q.layout_entries = q.layout_entries + 63ll * q.n;
            q.slotted = 1;
        }
        const char *fam = csr_kernel_family(q, f, slotted_now);
        const int ups = csr_updates_per_step(q);
        std::snprintf(buf, sizeof(buf),
                      "csr form=%s spins=%s waves=%d replicas_per_block=%d updates_per_step=%d slots=%d entries=%s table_m=%d "
                      "sstride=%d",
                      fam, f.bits ? "bits" : "int8", f.waves, csr_replicas_per_block(q, f),
                      std::strcmp(fam, "rows") == 0 ? ups : ((ups == 1 || ups == 2) && !f.bits && f.waves == 1 ? ups : 0),
                      slotted_now ? 1 : 0, (f.wants_packed && q.packed_ok) ? "packed" : "cv", f.table_m, f.sstride);
        out = buf;
        if (csr_shared(q)) {  // sga_set_csr_shared: one set of rows under n_models field vectors
            std::snprintf(buf, sizeof(buf), " shared-J models=%d", q.n_models);
            out += buf;
        }
        q.sstride = f.sstride;
    } else {
        const DenseGeometry g = dense_geometry(q);
        if (!g.fits) return "dense error=replica spins do not fit LDS (n too large)";
        const bool t2 = q.storage == SGA_J_T2, i8 = is_i8(q);
        const int W = t2 ? g.waves_t2 : g.waves, C = t2 ? g.cpw_t2 : g.cpw;
        const bool streaming = t2 ? C > sga::T2_MAX_CPW : C > sga::MAX_CPW;
        const int la = (q.table_m > 0 && q.opt[OPT_LOOK_AHEAD] != 0)
                           ? sga::dense_look_ahead(t2, i8, q.acc != 0 && !i8, C, W, std::max(q.R_local, 1)) : 1;
        std::snprintf(buf, sizeof(buf), "dense storage=%s acc=%s waves=%d chunks_per_wave=%d%s ld=%lld look_ahead=%d kernel=%s",
                      t2 ? "t2" : (i8 ? "i8" : "f32"), i8 ? "i32" : (q.acc == 0 ? "f32" : (q.acc == 2 ? "f64-canonical" : "f64-exact")),
                      W, C, streaming ? "(streaming)" : "", g.ld, la, t2 ? "sweep_dense_t2_kernel" : "sweep_dense_kernel");
        out = buf;
        if (q.shared_j && q.n_models > 1) {  // sga_set_dense_shared: one matrix under n_models field vectors
            std::snprintf(buf, sizeof(buf), " shared-J models=%d", q.n_models);
            out += buf;
        }
        // option "row_shared" = 1 forces the row-shared windows (sweep_dense_rs.hip) where the problem admits them, in the
        // integer class or -- option "row_shared_grid" = 1 -- on the binary grid of the set-time verdict (rs_grid = 1 + k);
        // the default 2 leaves the form to sga_autotune, which a query does not know about
        const sga_windows::WindowTraits wt = window_traits_of_query(q);
        if (const int w = sga_windows::row_shared_w(wt, true)) {
            if (const int grid = sga_windows::form_class(wt).grid)
                std::snprintf(buf, sizeof(buf), " sweep=row-shared(W=%d grid=2^-%d)", w, grid - 1);
            else
                std::snprintf(buf, sizeof(buf), " sweep=row-shared(W=%d)", w);
            out += buf;
        }
        q.sstride = (int)g.ld;
    }
    // what sga_set_field_cache would run
    if (q.field_cache == SGA_FIELD_CACHE_OFF) {
        out += " cached=off";
    } else {
        const char *why = clf_refusal(q);
        if (why) {
            out += q.field_cache == SGA_FIELD_CACHE_ON ? " cached=refused" : " cached=unavailable";
        } else if (q.field_cache == SGA_FIELD_CACHE_ON) {
            if (csr_ragged(q) && q.opt[OPT_CLF_FIXED_POINT] == 1 && (q.clf_bits == 32 || q.clf_bits == 64))
                std::snprintf(buf, sizeof(buf), " cached=on(waves=%d fields=int%d fixed-point models=%d)", clf_csr_waves(q), q.clf_bits,
                              q.n_models);
            else if (q.kind == SGA_ROUTE_CSR && q.opt[OPT_CLF_FIXED_POINT] == 1 && (q.clf_bits == 32 || q.clf_bits == 64))
                std::snprintf(buf, sizeof(buf), " cached=on(waves=%d fields=int%d fixed-point)", clf_csr_waves(q), q.clf_bits);
            else if (dense_fixed_point(q) && q.n_models > 1 && q.opt[OPT_BATCH_FIXED_POINT] == 1)
                // a many-model dense batch under option "batch_fixed_point": batch-wide k and field width, each replica on
                // its model's rows (sweep_clf_fx.hip, MODELS)
                std::snprintf(buf, sizeof(buf), " cached=on(waves=%d fields=int%d fixed-point models=%d)",
                              sga::sweep_clf_waves(dense_ldj(q), is_i8(q), std::max(q.R_local, 1), q.cus, (int)q.opt[OPT_CLF_WAVES]),
                              q.clf_bits, q.n_models);
            else if (dense_fixed_point(q))
                std::snprintf(buf, sizeof(buf), " cached=on(waves=%d fields=int%d fixed-point)",
                              sga::sweep_clf_waves(dense_ldj(q), is_i8(q), std::max(q.R_local, 1), q.cus, (int)q.opt[OPT_CLF_WAVES]),
                              q.clf_bits);
            else if (csr_ragged(q))  // a ragged batch: waves by its longest row and largest model
                std::snprintf(buf, sizeof(buf), " cached=on(waves=%d models=%d)", clf_csr_waves(q), q.n_models);
            else if (q.kind == SGA_ROUTE_CSR) std::snprintf(buf, sizeof(buf), " cached=on(waves=%d)", clf_csr_waves(q));
            else if (q.n_models > 1)  // a many-model dense batch: batch-wide field width, each replica on its model's rows
                std::snprintf(buf, sizeof(buf), " cached=on(waves=%d fields=int%d models=%d)",
                              sga::sweep_clf_waves(dense_ldj(q), is_i8(q), std::max(q.R_local, 1), q.cus, (int)q.opt[OPT_CLF_WAVES]),
                              q.clf_bits, q.n_models);
            else
                std::snprintf(buf, sizeof(buf), " cached=on(waves=%d fields=int%d)",
                              sga::sweep_clf_waves(dense_ldj(q), is_i8(q), std::max(q.R_local, 1), q.cus, (int)q.opt[OPT_CLF_WAVES]),
                              q.clf_bits);
            out += buf;
        } else {
            if (q.n_models > 1)  // (CSR: a ragged batch under option "ragged_field_cache")
                std::snprintf(buf, sizeof(buf), " cached=auto(start=%s theta=%.3f models=%d)", auto_starts_cached(q) ? "cached" : "rows",
                              routing_theta(q), q.n_models);
            else
                std::snprintf(buf, sizeof(buf), " cached=auto(start=%s theta=%.3f)", auto_starts_cached(q) ? "cached" : "rows",
                              routing_theta(q));
            out += buf;
        }
    }
    return out;
}

}  // namespace sga_route

extern "C" {

int sga_route_query_init(sga_route_query *q) {
    if (!q) return sga_impl::fail(SGA_ERR_INVALID, "query is NULL");
    std::memset(q, 0, sizeof(*q));
    q->n_models = 1;
    q->cus = 256;
    q->table_scale = 1;
    q->clf_bits = 16;
    q->clf_scale = 1;
    q->rowptr32 = 1;
    for (int i = 0; i < sga_impl::OPT_COUNT; ++i) q->opt[i] = sga_impl::OPT_DEFS[i].def;
    return SGA_OK;
}

int sga_explain_route(const sga_route_query *q, char *buf, int buflen) {
    if (!q || !buf || buflen <= 0) return sga_impl::fail(SGA_ERR_INVALID, "bad arguments");
    if (q->n <= 0 || q->kind < SGA_ROUTE_DENSE || q->kind > SGA_ROUTE_GROUPS || (q->kind == SGA_ROUTE_TSP && q->n_cities < 3) ||
        (q->kind == SGA_ROUTE_GROUPS && (q->n_groups < 0 || (q->n_groups < 1 && q->rest_nnz < 1))))
        return sga_impl::fail(SGA_ERR_INVALID, "route query: kind / n out of range");
    std::snprintf(buf, (size_t)buflen, "%s", sga_route::explain(*q).c_str());
    return SGA_OK;
}

}  // extern "C"
