// sga_quantum.cpp -- simulated quantum annealing, the engine half (the pure half: sga_quantum.h): sga_sweep_transverse,
// sga_sweep_transverse_dense, sga_worldline_clusters, sga_worldline_clusters_dense, sga_get_time_links and
// sga_exchange_transverse.  None keeps state of its own: the caller's host array is staged in scratch slot 0 (where
// sga_sweep stages a schedule) by stage_host, results leave through DevOut / deliver (sga_engine_impl.h), as those of the
// replica calls of sga_replicas.cpp do.  A sweep is two launches on the engine's stream, the even slices' half-sweep and
// the odd ones'; one launch serves a whole clusters call.
#include "sga_engine_impl.h"

namespace {

// What of an engine the admission rules read (no engine: the defaults, the rules say so first).
sga::TrotterProblem trotter_problem_of(const sga_engine *e) {
    sga::TrotterProblem p;
    if (!e) return p;
    p.n = e->n, p.R_local = e->spins ? e->R : 0, p.replica0 = e->replica0, p.sstride = e->sstride;
    p.csr = e->csr, p.tsp = e->tsp, p.groups = e->groups, p.ragged = e->ragged, p.n_models = e->n_models;
    p.metropolis = e->rule == SGA_RULE_METROPOLIS;
    p.csr_acc = e->csr_acc;
    p.consistent_dE = e->consistent_dE;
    p.clf_problem = (!e->csr && !e->implicit() && e->clf_problem && !e->clf_fx_bits) ? 1 : 0;
    p.clf_why = e->clf_why;
    p.field_bits = e->clf_bits;
    p.ldf = (e->ldj + 127) / 128 * 128;  // (as ensure_fields lays the rows out)
    // (option "clf_fixed_point", read when the couplings were set: the verdict on a dense problem the integer form refused)
    if (!e->csr && !e->implicit() && !e->clf_problem) p.fx_bits = e->clf_fx_bits, p.fx_why = e->clf_fx_why;
    p.R_global = e->Rg;
    return p;
}

// The bytes of a replica's resident field row, whichever form seeded it (ensure_fields): ldf is a multiple of 128.
long long field_row_bytes_of(const sga_engine *e) {
    const int bits = e->clf_fx_bits ? e->clf_fx_bits : e->csr ? 16 : e->clf_bits;
    return e->ldf * (long long)(bits / 8);
}

// From the admission rule's answer to the device: run = true where the call goes on, else the returned code is the call's.
int begin_call(sga_engine *e, const char *why, bool invalid, int n_sweeps, bool &run) {
    run = false;
    if (why) return fail(invalid ? SGA_ERR_INVALID : SGA_ERR_UNSUPPORTED, why);
    if (n_sweeps == 0) return SGA_OK;
    if (e->opt_stale)
        return fail(SGA_ERR_INVALID, std::string("option \"") + (e->opt_stale_key ? e->opt_stale_key : "?") +
                                         "\" changed after it was read: set the couplings and initialise the replicas again");
    if ((e->csr ? !e->rowptr64 || !e->cv : !e->J_packed) || !e->h || !e->best_spins) return fail(SGA_ERR_INVALID, "no couplings set");
    HIPCHK(hipSetDevice(e->device));
    run = true;
    return SGA_OK;
}

// The caller's host array at the base of scratch slot 0, `behind` bytes reserved after it, 8-byte aligned, at *behind_at.
int stage(sga_engine *e, const void *host, size_t bytes, size_t behind = 0, size_t *behind_at = nullptr) {
    const size_t padded = (bytes + 7) / 8 * 8;
    if (behind_at) *behind_at = padded;
    return stage_host(e->scratch[0], padded + behind, 0, host, bytes, e->stream);
}

// A launch that did not go out: nothing is known about the sweep's state, the fields, or which rows were traded.
int launched(sga_engine *e, hipError_t le) {
    if (le != hipSuccess) {
        (void)hipStreamSynchronize(e->stream);
        e->fields_valid = false;
    }
    HIPCHK(le);
    return SGA_OK;
}

// What every launch reads of the replicas and the random stream; the caller adds its view of the couplings.
sga::SweepArgs replica_args_of(const sga_engine *e) {
    sga::SweepArgs a{};
    a.h = e->h, a.spins = e->spins, a.best_spins = e->best_spins;
    a.energy = e->energy, a.best_energy = e->best_energy, a.rep_temp = e->rep_temp;
    geometry_into(a, e);
    seed_into(a, e);
    return a;
}

// The n_sweeps sweeps of either sweep call: k_perp staged, then per sweep the two half-sweeps through `launch`.
template <typename Launch>
int run_half_sweeps(sga_engine *e, sga::SweepArgs a, int n_sweeps, int n_slices, int arith, const float *k_perp, Launch launch) {
    const int G = e->R / n_slices;
    const int rc = stage(e, k_perp, (size_t)n_sweeps * (size_t)G * sizeof(float));
    if (rc != SGA_OK) return rc;
    const float *d_k = slot_at<const float>(e->scratch[0]);
    a.n_accepted = e->n_acc;
    a.n_sweeps = 1, a.site_mode = SGA_SITE_RANDOM, a.arith = arith, a.rule = SGA_RULE_METROPOLIS;
    for (int kk = 0; kk < n_sweeps; ++kk) {
        a.sweep0 = e->sweeps_done + (uint32_t)kk;
        for (int parity = 0; parity < 2; ++parity) {
            const sga::TrotterLaunch t{d_k + (size_t)kk * (size_t)G, n_slices, parity, G * (n_slices / 2)};
            if (const int rc = launched(e, launch(a, t))) return rc;
        }
    }
    std::snprintf(e->last_kernel, sizeof(e->last_kernel), "%s", sga::last_sweep_kernel());
    e->sweeps_done += (uint32_t)n_sweeps;
    e->attempted += (long long)n_sweeps * e->n;
    return SGA_OK;
}

bool arith_ok(int arith) { return arith == SGA_ARITH_F64 || arith == SGA_ARITH_F32; }

}  // namespace

int sga_sweep_transverse(sga_engine *e, int n_sweeps, int n_slices, int arith, const float *k_perp) {
    if (const int rc = refuse_device_ptr(k_perp, "k_perp")) return rc;
    bool invalid = true, run = false;
    const char *why = sga::transverse_check(e != nullptr, trotter_problem_of(e), n_sweeps, n_slices, arith_ok(arith), k_perp, &invalid);
    const int rc = begin_call(e, why, invalid, n_sweeps, run);
    if (!run) return rc;
    sga::SweepArgs a = replica_args_of(e);
    a.rowptr64 = e->rowptr64, a.cv = e->cv, a.diag = e->diag, a.csr_acc = e->csr_acc;
    e->fields_valid = false;  // (as after sga_set_spins: the next sweep seeds the cached fields again)
    return run_half_sweeps(e, a, n_sweeps, n_slices, arith, k_perp,
                           [&](const sga::SweepArgs &s, const sga::TrotterLaunch &t) { return sga::launch_sweep_transverse(s, t, e->stream); });
}

// The resident fields of the dense cached-field sweep carry the step: seeded through ensure_fields where they are not
// valid, written back by every launch for the slices that moved -- they stay valid.
int sga_sweep_transverse_dense(sga_engine *e, int n_sweeps, int n_slices, int arith, const float *k_perp) {
    if (const int rc = refuse_device_ptr(k_perp, "k_perp")) return rc;
    bool invalid = true, run = false;
    const char *why = sga::transverse_dense_check(e != nullptr, trotter_problem_of(e), n_sweeps, n_slices, arith_ok(arith), k_perp, &invalid);
    int rc = begin_call(e, why, invalid, n_sweeps, run);
    if (!run) return rc;
    // (SGA_FIELD_CACHE_AUTO routes replica by replica: the fields of a replica on the row kernels are stale while
    //  fields_valid stands for the others -- this call reads every slice's, so under AUTO it seeds them itself)
    if (e->field_cache == SGA_FIELD_CACHE_AUTO) e->fields_valid = false;
    rc = ensure_fields(e);
    if (rc != SGA_OK) return rc;
    sga::SweepArgs a = replica_args_of(e);
    a.J = e->J_packed, a.ldj = e->ldj;
    // (fixed-point fields, option "clf_fixed_point": D = 2^k J s as int32 | int64, seeded by dense_fields_seed_fx_kernel)
    const bool fx = e->clf_fx_bits != 0;
    a.fields = e->fields, a.ldf = e->ldf;
    a.field_bits = fx ? e->clf_fx_bits : e->clf_bits, a.field_scale = fx ? e->clf_fx_k : e->clf_scale;
    // waves per slice: option "clf_waves", else the cached-field sweep's choice over the workgroups of a launch, R / 2
    const int waves = sga::sweep_clf_waves(e->ldj, e->want_i8, e->R / 2, e->cus, (int)e->opt[OPT_CLF_WAVES]);
    return run_half_sweeps(e, a, n_sweeps, n_slices, arith, k_perp, [&](const sga::SweepArgs &s, const sga::TrotterLaunch &t) {
        return fx ? sga::launch_sweep_transverse_dense_fx(s, t, e->want_i8, waves, e->stream)
                  : sga::launch_sweep_transverse_dense(s, t, e->want_i8, waves, e->stream);
    });
}

namespace {

// Either world-line call: the thresholds floor(p_bond 2^24), formed here in double, are staged with the group counts
// behind them; one launch; the counts are added to the caller's.  What differs comes in: the admission rule, whether the
// step is decided on the resident fields (on_fields), the call's view of the couplings and its launch.
template <typename Check, typename View, typename Launch>
int worldline_call(sga_engine *e, int n_sweeps, int n_slices, uint32_t round, const double *p_bond, int64_t *stats, Check check,
                   bool on_fields, View view, Launch launch) {
    if (const int rc = refuse_device_ptr(p_bond, "p_bond")) return rc;
    if (const int rc = refuse_device_ptr(stats, "stats")) return rc;
    bool invalid = true, run = false;
    const char *why = check(e != nullptr, trotter_problem_of(e), n_sweeps, n_slices, p_bond, &invalid);
    int rc = begin_call(e, why, invalid, n_sweeps, run);
    if (!run) return rc;
    if (on_fields) {
        // (SGA_FIELD_CACHE_AUTO: some replicas' fields may be stale while fields_valid stands, as in sga_sweep_transverse_dense)
        if (e->field_cache == SGA_FIELD_CACHE_AUTO) e->fields_valid = false;
        rc = ensure_fields(e);
        if (rc != SGA_OK) return rc;
    }
    hipStream_t st = e->stream;
    const int G = e->R / n_slices;
    std::vector<uint32_t> thr((size_t)n_sweeps * (size_t)G);
    for (size_t i = 0; i < thr.size(); ++i) thr[i] = sga::worldline_threshold(p_bond[i]);
    DevOut<int64_t> counts(stats, (size_t)G * 3, 0, 0, true);  // (a device buffer was refused above: added up on the host)
    size_t counts_at = 0;
    rc = stage(e, thr.data(), thr.size() * sizeof(uint32_t), counts.bytes(), &counts_at);
    if (rc != SGA_OK) return rc;
    if (stats) counts.staged(slot_at<void>(e->scratch[0], counts_at));
    sga::SweepArgs a = replica_args_of(e);
    view(a);
    const sga::WorldlineArgs w{slot_at<const uint32_t>(e->scratch[0]), reinterpret_cast<long long *>(counts.ptr), n_slices, n_sweeps, round};
    // (the sparse step leaves the fields behind, as sga_set_spins does; the dense one keeps them valid unless its launch fails)
    if (!on_fields) e->fields_valid = false;
    if ((rc = launched(e, launch(a, w, st))) != SGA_OK) return rc;
    std::snprintf(e->last_kernel, sizeof(e->last_kernel), "%s", sga::last_sweep_kernel());
    return deliver(st, counts);
}

}  // namespace

int sga_worldline_clusters(sga_engine *e, int n_sweeps, int n_slices, uint32_t round, const double *p_bond, int64_t *stats) {
    return worldline_call(
        e, n_sweeps, n_slices, round, p_bond, stats, sga::worldline_check, false,
        [&](sga::SweepArgs &a) { a.rowptr64 = e->rowptr64, a.cv = e->cv, a.csr_acc = e->csr_acc; },
        [&](const sga::SweepArgs &a, const sga::WorldlineArgs &w, hipStream_t st) { return sga::launch_worldline_clusters(a, w, st); });
}

// The step of sga_worldline_clusters on the dense rows, decided on the resident fields of every slice: seeded through
// ensure_fields where they are not valid, updated by the launch for every flip -- they stay valid.
int sga_worldline_clusters_dense(sga_engine *e, int n_sweeps, int n_slices, uint32_t round, const double *p_bond, int64_t *stats) {
    return worldline_call(
        e, n_sweeps, n_slices, round, p_bond, stats, sga::worldline_dense_check, true,
        [&](sga::SweepArgs &a) {
            a.J = e->J_packed, a.ldj = e->ldj;
            a.fields = e->fields, a.ldf = e->ldf, a.field_bits = e->clf_bits, a.field_scale = e->clf_scale;
        },
        [&](const sga::SweepArgs &a, const sga::WorldlineArgs &w, hipStream_t st) {
            return sga::launch_worldline_clusters_dense(a, w, e->want_i8, sga::worldline_dense_waves(e->ldj, e->want_i8, (int)e->opt[OPT_CLF_WAVES]), st);
        });
}

// ---- the exchange between groups along the transverse field (trotter_exchange.hip) ----------------------------------------
// Read only: the counts go into the caller's device buffer, or through scratch slot 0 onto the host.
int sga_get_time_links(sga_engine *e, int n_slices, int64_t *links) {
    bool invalid = true;
    if (const char *why = sga::time_links_check(e != nullptr, trotter_problem_of(e), n_slices, links, &invalid))
        return fail(invalid ? SGA_ERR_INVALID : SGA_ERR_UNSUPPORTED, why);
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    DevOut<int64_t> out(links, (size_t)(e->R / n_slices));
    if (const int rc = out.direct(e->scratch[0])) return rc;
    HIPCHK(hipMemsetAsync(out.ptr, 0, out.bytes(), st));
    HIPCHK(sga::launch_time_links(e->spins, e->sstride, e->R, n_slices, reinterpret_cast<long long *>(out.ptr), st));
    std::snprintf(e->last_kernel, sizeof(e->last_kernel), "%s", sga::last_sweep_kernel());
    return deliver(st, out);
}

// k_perp is staged in scratch slot 0 with the counts and the flags behind it; the counts, the decision, the swap and the
// bests' step follow each other on the engine's stream.  The resident fields are traded with the spins where they are
// valid, and stay valid -- under SGA_FIELD_CACHE_AUTO, where fields_valid stands for some replicas only, they are marked
// for re-seeding instead.
int sga_exchange_transverse(sga_engine *e, int n_slices, const float *k_perp, int parity, uint32_t round, int32_t *accepted, int64_t *links) {
    if (const int rc = refuse_device_ptr(k_perp, "k_perp")) return rc;
    bool invalid = true;
    if (const char *why = sga::exchange_check(e != nullptr, trotter_problem_of(e), n_slices, k_perp, parity, &invalid))
        return fail(invalid ? SGA_ERR_INVALID : SGA_ERR_UNSUPPORTED, why);
    if (!e->best_spins || !e->energy || !e->best_energy || !e->rep_temp) return fail(SGA_ERR_INVALID, "no replicas (call sga_init_replicas)");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const size_t G = (size_t)(e->R / n_slices);
    size_t behind = 0;
    if (const int rc = stage(e, k_perp, G * sizeof(float), G * (sizeof(int64_t) + sizeof(int32_t)), &behind)) return rc;
    DevOut<int32_t> out_accepted(accepted, G);
    DevOut<int64_t> out_links(links, G);
    out_links.staged(slot_at<void>(e->scratch[0], behind));
    out_accepted.staged(slot_at<void>(e->scratch[0], behind + G * sizeof(int64_t)));
    long long *d_links = reinterpret_cast<long long *>(out_links.ptr);
    if (e->field_cache == SGA_FIELD_CACHE_AUTO) e->fields_valid = false;
    const bool trade_fields = e->fields_valid && e->fields;
    const sga::SweepArgs a = replica_args_of(e);
    const sga::TrotterExchangeArgs x{slot_at<const float>(e->scratch[0]), d_links, out_accepted.ptr, n_slices, parity, round,
                                     trade_fields ? e->fields : nullptr, trade_fields ? field_row_bytes_of(e) : 0};
    HIPCHK(hipMemsetAsync(d_links, 0, G * sizeof(int64_t), st));
    HIPCHK(sga::launch_time_links(e->spins, e->sstride, e->R, n_slices, d_links, st));
    HIPCHK(sga::launch_trotter_exchange_decide(a, x, st));
    hipError_t le = sga::launch_trotter_exchange_swap(a, x, st);
    std::snprintf(e->last_kernel, sizeof(e->last_kernel), "%s", sga::last_sweep_kernel());
    if (le == hipSuccess) le = sga::launch_update_best(e->energy, e->spins, e->best_energy, e->best_spins, e->sstride, e->R, st);
    if (const int rc = launched(e, le)) return rc;
    return deliver(st, out_accepted, out_links);
}
