// sga_engine.cpp -- host side of the C ABI declared in include/sga.h: owns the HBM buffers
// (packed couplings, replica spins / energies / bests, ladder state), picks the launch
// geometry, and drives the HIP kernels.  No torch, no exceptions across the ABI.
// (problem set-up: sga_problem.cpp; autotune: sga_autotune.cpp; state access / describe: sga_state.cpp; form selection:
// sga_route.cpp; the window forms' admission, state and scratch: sga_windows.cpp; shared internals: sga_engine_impl.h)
#include "sga_engine_impl.h"

#include <cmath>
#include <cstdio>

namespace sga_impl {

sga_route_query route_query_of(const sga_engine *e) {
    sga_route_query q;
    (void)sga_route_query_init(&q);
    q.kind = e->groups ? SGA_ROUTE_GROUPS : e->tsp ? SGA_ROUTE_TSP : (e->csr ? SGA_ROUTE_CSR : SGA_ROUTE_DENSE);
    q.n = e->n;
    q.n_models = e->n_models;
    q.shared_j = e->shared_j ? 1 : 0;
    q.R_local = e->R;
    q.cus = e->cus;
    q.tune_waves = e->tune_waves;
    q.field_cache = e->field_cache;
    if (e->csr) {
        q.storage = e->csr_storage;
        q.acc = e->csr_acc;
        q.clf_ok = e->clf_csr_problem ? 1 : 0;
    } else {
        q.storage = e->use_t2 ? SGA_J_T2 : (e->want_i8 ? SGA_J_I8 : SGA_J_F32);
        q.acc = e->acc64 ? (e->acc_canon ? 2 : 1) : 0;
        q.clf_ok = e->clf_problem ? 1 : 0;
    }
    q.table_m = e->table_m;
    q.table_scale = e->table_scale;
    q.clf_bits = e->clf_bits;
    q.clf_scale = e->clf_scale;
    // option "clf_fixed_point": CSR queries carry the width of the fixed-point fields (32 | 64; 16: the int16 form)
    if (e->csr && e->opt[OPT_CLF_FIXED_POINT] == 1) q.clf_bits = e->clf_fx_bits ? e->clf_fx_bits : 16;
    // ... dense queries whose problem the integer form does not take: 32 | 64, 0 = refused (sga_route.cpp, dense_fixed_point)
    if (!e->csr && !e->implicit() && e->opt[OPT_CLF_FIXED_POINT] == 1 && !e->clf_problem) q.clf_bits = e->clf_fx_bits;
    q.from_dense = e->from_dense ? 1 : 0;
    q.nnz = e->nnz;
    q.max_row_len = e->max_row_len;
    q.layout_entries = e->layout_entries;
    q.slotted = e->slotted ? 1 : 0;
    q.rowptr32 = e->rowptr ? 1 : 0;
    q.packed_ok = e->cvp ? 1 : 0;
    q.n_cities = e->tsp ? e->tsp_args.n_cities : 0;
    q.n_groups = e->groups ? e->group_args.n_groups : 0;
    q.group_max = e->groups ? e->g_max_size : 0;
    q.rest_nnz = e->groups ? e->group_args.rest.nnz : 0;
    q.rest_max_row = e->groups ? e->group_args.rest.max_row : 0;
    q.rs_grid = (!e->csr && !e->implicit() && e->win.grid_planes > 0) ? 1 + e->win.grid_k : 0;
    q.sstride = e->sstride;
    q.ldj = e->ldj;
    for (int i = 0; i < OPT_COUNT; ++i) q.opt[i] = e->opt[i];
    return q;
}

// All replicas' local fields in one pass over the couplings on the matrix cores (fields_dense.hip),
// then energies and / or the resident fields of the cached-field sweep from them.
bool fields_pass_applies(const sga_engine *e, int count) {
    // option "batched_energy": 0 = off (A/B switch), 1 = where the batched sums carry the same bits as the
    // per-replica kernels', 2 = always.  The finish pass adds X and Y in the per-replica kernels' order
    // (energy_block_rows), so the energies agree bit for bit wherever the row sums do.  Real-valued couplings that
    // need the canonical summation order keep the per-replica kernels under 1: the matrix-core pass sums a row in
    // k-order, and the fp32-rounded row sum could differ in its last bit with the number of replicas recomputed
    // together (sga_set_spins: one; a shard: R_local).
    const long long mode = e->opt[OPT_BATCHED_ENERGY];
    if (mode == 0 || (mode == 1 && e->acc_canon)) return false;
    // (one matrix for every replica: one model, or the models of sga_set_dense_shared -- the finish pass reads each
    //  replica's own h)
    return !e->csr && !e->implicit() && (e->n_models == 1 || e->shared_j) && count >= 32 && e->J_packed;
}
// The pass writes Y = S J^T for the replicas it is given into a scratch buffer ([tile][ldj] int32 | fp32) before
// the finish kernel reduces it.  The scratch is bounded: replica sets whose Y would exceed the cap go
// through in tiles of whole 128-replica blocks (option "fields_scratch_mb", 256; one more pass over J per tile: 16 384 replicas of 10 000 spins =
// three passes over 100 MB instead of 655 MB of scratch kept for the life of the replicas), and a failed
// allocation halves the tile before giving up with SGA_ERR_MEMORY -- which the callers treat as "this fast path is
// not available" (per-replica energy kernels; SGA_FIELD_CACHE_AUTO stays on the row-per-proposal kernels).
int fields_pass(sga_engine *e, int r0, int count, double *energy, void *fields) {
    const size_t row = sizeof(float) * (size_t)e->ldj;
    long long tile = count;
    const size_t scratch_cap = (size_t)e->opt[OPT_FIELDS_SCRATCH_MB] << 20;  // option "fields_scratch_mb" (256)
    const long long cap_rows = std::max<long long>(128, (long long)(scratch_cap / row) / 128 * 128);
    if (tile > cap_rows) tile = cap_rows;
    while (row * (size_t)tile > e->ybuf_bytes) {
        dev_free(e->ybuf);
        e->ybuf_bytes = 0;
        if (hipMalloc(&e->ybuf, row * (size_t)tile) == hipSuccess) {
            e->ybuf_bytes = row * (size_t)tile;
            break;
        }
        (void)hipGetLastError();  // (cleared: the caller may go on without this pass)
        e->ybuf = nullptr;
        if (tile <= 128) return fail(SGA_ERR_MEMORY, "no memory for the scratch of the all-replica field pass");
        tile = std::max<long long>(128, tile / 2 / 128 * 128);
    }
    const int mode = e->want_i8 ? 0 : (e->acc64 ? 2 : 1);
    const size_t fbytes = (size_t)(e->clf_bits / 8);
    for (long long t0 = 0; t0 < count; t0 += tile) {
        sga::FieldsArgs f{};
        f.J = e->J_packed;
        f.spins = e->spins + (long long)(r0 + t0) * e->sstride;
        f.Y = e->ybuf;
        f.h = e->h;
        f.energy = energy ? energy + t0 : nullptr;
        f.fields = fields ? static_cast<unsigned char *>(fields) + (size_t)t0 * (size_t)e->ldf * fbytes : nullptr;
        f.ldj = e->ldj;
        f.ldy = e->ldj;
        f.ldf = e->ldf;
        f.n = e->n;
        f.R = (int)std::min<long long>(tile, count - t0);
        f.sstride = e->sstride;
        f.field_bits = fields ? e->clf_bits : 0;
        f.field_scale = e->clf_scale;
        f.eblock = sga::energy_block_rows(e->n);
        f.reps_per_model = e->shared_j ? e->Rg / e->n_models : 0;
        f.replica_base = e->replica0 + r0 + (int)t0;
        HIPCHK(sga::launch_fields_dense(f, mode, e->stream));
        HIPCHK(sga::launch_fields_finish(f, mode == 0, e->stream));
    }
    return SGA_OK;
}

// The cached-local-field sweep serves this problem / these replicas?  why: the reason when it does not
// (sga_route.cpp, clf_refusal).
bool clf_possible(const sga_engine *e, const char **why) {
    const sga_route_query q = route_query_of(e);
    const char *reason = sga_route::clf_refusal(q);
    // (option "clf_fixed_point": the set-time scan knows which condition failed; the query carries only the verdict)
    if (reason && !q.clf_ok && e->clf_fx_why && (!e->csr || q.n_models == 1)) reason = e->clf_fx_why;
    // (the integer form over dense couplings, likewise)
    if (reason && !q.clf_ok && !e->csr && !e->implicit() && e->clf_why && e->opt[OPT_CLF_FIXED_POINT] != 1) reason = e->clf_why;
    // (ragged CSR batches under option "ragged_field_cache": the first offending model and the condition it fails)
    if (reason && !q.clf_ok && e->ragged && !e->clf_ragged_why.empty()) reason = e->clf_ragged_why.c_str();
    if (why) *why = reason;
    return reason == nullptr;
}
bool clf_active(const sga_engine *e) {
    return e->field_cache != SGA_FIELD_CACHE_OFF && e->rule != SGA_RULE_WOLFF && clf_possible(e, nullptr);
}
// resident fields of every replica, from the all-replica pass (the tracked energies are left alone)
int ensure_fields(sga_engine *e) {
    if (e->fields_valid && e->fields) return SGA_OK;
    if (e->ragged) {  // D = J_m s of every replica over its model's rows, up to eight replicas of a model per pass
        e->ldf = ((long long)e->n + 127) / 128 * 128;  // (the largest model's)
        const size_t fbytes = e->clf_fx_bits ? (size_t)(e->clf_fx_bits / 8) : 2;  // (fixed point: D = 2^k J_m s, int32 | int64)
        if (!e->fields && hipMalloc(&e->fields, (size_t)e->R * (size_t)e->ldf * fbytes) != hipSuccess) {
            (void)hipGetLastError();
            e->fields = nullptr;
            return fail(SGA_ERR_MEMORY, "no memory for the resident local fields of the cached-field sweep");
        }
        if (e->clf_fx_bits) {  // options "ragged_field_cache" and "clf_fixed_point": exact sums at the batch-wide k, h not folded in
            HIPCHK(sga::launch_csr_fields_seed_ragged_fx(e->rowptr64, e->cv, e->spins, e->sstride, e->n, e->R,
                                                         (unsigned int)e->replica0, e->Rg / e->n_models, e->d_models, e->fields,
                                                         e->ldf, e->clf_fx_bits, e->clf_fx_k, e->stream));
            e->fields_valid = true;
            return SGA_OK;
        }
        if (!e->hq) {  // scale * h of every row of the concatenation, at the batch-wide scale
            HIPCHK(hipMalloc(&e->hq, sizeof(int) * (size_t)e->n_rows));
            HIPCHK(sga::launch_scaled_fields(e->h, e->n_rows, e->table_scale, e->hq, e->stream));
        }
        HIPCHK(sga::launch_csr_fields_seed_ragged(e->rowptr64, e->cv, e->spins, e->sstride, e->n, e->R, (unsigned int)e->replica0,
                                                  e->Rg / e->n_models, e->d_models, static_cast<short *>(e->fields), e->ldf,
                                                  e->stream));
        e->fields_valid = true;
        return SGA_OK;
    }
    if (e->csr) {  // D = J s of every replica (int16), eight replicas per pass over the entries; scale * h once
        e->ldf = ((long long)e->n + 127) / 128 * 128;
        const size_t fbytes = e->clf_fx_bits ? (size_t)(e->clf_fx_bits / 8) : 2;  // (fixed point: D = 2^k J s, int32 | int64)
        if (!e->fields && hipMalloc(&e->fields, (size_t)e->R * (size_t)e->ldf * fbytes) != hipSuccess) {
            (void)hipGetLastError();
            e->fields = nullptr;
            return fail(SGA_ERR_MEMORY, "no memory for the resident local fields of the cached-field sweep");
        }
        if (e->clf_fx_bits) {
            HIPCHK(sga::launch_csr_fields_seed_fx(e->rowptr64, e->cv, e->spins, e->sstride, e->n, e->R, e->fields, e->ldf,
                                                  e->clf_fx_bits, e->clf_fx_k, e->stream));
            e->fields_valid = true;
            return SGA_OK;
        }
        if (!e->hq) {
            HIPCHK(hipMalloc(&e->hq, sizeof(int) * (size_t)e->n));
            HIPCHK(sga::launch_scaled_fields(e->h, e->n, e->table_scale, e->hq, e->stream));
        }
        HIPCHK(sga::launch_csr_fields_seed(e->rowptr64, e->cv, e->spins, e->sstride, e->n, e->R,
                                           static_cast<short *>(e->fields), e->ldf, e->stream));
        e->fields_valid = true;
        return SGA_OK;
    }
    e->ldf = (e->ldj + 127) / 128 * 128;
    const int fbits = e->clf_fx_bits ? e->clf_fx_bits : e->clf_bits;  // (fixed point: D = 2^k J s, int32 | int64)
    if (!e->fields && hipMalloc(&e->fields, (size_t)e->R * (size_t)e->ldf * (size_t)(fbits / 8)) != hipSuccess) {
        (void)hipGetLastError();
        e->fields = nullptr;
        return fail(SGA_ERR_MEMORY, "no memory for the resident local fields of the cached-field sweep");
    }
    if (e->clf_fx_bits && e->n_models > 1) {  // option "batch_fixed_point": each replica over its own model's rows
        HIPCHK(sga::launch_dense_fields_seed_fx_batch(e->J_packed, e->want_i8, e->ldj, model_stride_j(e), e->spins,
                                                      e->sstride, e->n, e->R, (uint32_t)e->replica0, e->Rg / e->n_models,
                                                      e->fields, e->ldf, e->clf_fx_bits, e->clf_fx_k, e->stream));
        e->fields_valid = true;
        return SGA_OK;
    }
    if (e->clf_fx_bits) {  // exact per-replica sums (the matrix-core pass rounds real-valued row sums to fp32)
        HIPCHK(sga::launch_dense_fields_seed_fx(e->J_packed, e->want_i8, e->ldj, e->spins, e->sstride, e->n, e->R, e->fields,
                                                e->ldf, e->clf_fx_bits, e->clf_fx_k, e->stream));
        e->fields_valid = true;
        return SGA_OK;
    }
    // many-model batches: exact integer sums per model, one launch (sweep_clf.hip).  One shared matrix holding 32
    // replicas or more: the matrix-core pass below, J read once for all of them (integer sums: the same fields)
    if (e->n_models > 1 && !(e->shared_j && e->R >= 32)) {
        HIPCHK(sga::launch_dense_fields_seed_batch(e->J_packed, e->want_i8, e->ldj, model_stride_j(e), e->h, e->spins,
                                                   e->sstride, e->n, e->R, (uint32_t)e->replica0, e->Rg / e->n_models,
                                                   e->fields, e->ldf, e->clf_bits, e->clf_scale, e->stream));
        e->fields_valid = true;
        return SGA_OK;
    }
    int rc = fields_pass(e, 0, e->R, nullptr, e->fields);  // (any replica count: short tiles are clamped)
    if (rc != SGA_OK) return rc;
    e->fields_valid = true;
    return SGA_OK;
}

int recompute_energy_range(sga_engine *e, int r0, int count) {
    if (fields_pass_applies(e, count)) {
        const int rc = fields_pass(e, r0, count, e->energy + r0, nullptr);
        if (rc != SGA_ERR_MEMORY) return rc;  // (no room for its scratch: the per-replica kernels below need none)
    }
    const long long batched = e->opt[OPT_BATCHED_ENERGY];  // (one switch for both passes)
    // (the pass adds X = sum_i mv_i s_i in an order of its own: under 1 only where X is exact in fp64, csr_x_exact)
    const bool csr_all = batched == 2 || (batched == 1 && e->csr_x_exact);
    if (e->ragged) {  // ragged CSR batches: one workgroup per replica over its model's rows
        sga::EnergyArgs a{};
        a.rowptr = e->rowptr64;
        a.cv = e->cv;
        a.h = e->h;
        a.spins = e->spins + (long long)r0 * e->sstride;
        a.energy = e->energy + r0;
        a.n = e->n;
        a.sstride = e->sstride;
        a.R = count;
        a.reps_per_model = e->Rg / e->n_models;
        a.replica_base = e->replica0 + r0;
        a.slices = 1;
        HIPCHK(sga::launch_energy_csr_ragged(a, e->d_models, e->stream));
        return SGA_OK;
    }
    if (e->csr && !e->implicit() && count >= 64 && csr_all) {
        // all replicas in one pass over the entries: spins transposed to bits, 32 replicas per lane
        // row groups: enough (group, replica word) threads to fill the chip -- ~4 waves per SIMD -- whatever
        // the replica count (256 replicas = 8 words: 4096 groups left half the SIMDs without a wave)
        const int words = (count + 31) / 32;
        const int groups = std::max(1, std::min(e->n, std::max(1024, 262144 / words)));
        if (e->csr_energy.reserve(sga::csr_energy_scratch_bytes(e->n, count, groups)) == hipSuccess) {
            const bool exact32 = e->csr_acc == sga::CSR_ACC_F32_TABLE || e->csr_acc == sga::CSR_ACC_F32;
            HIPCHK(sga::launch_energy_csr_all(e->rowptr64, e->cv, e->h, e->spins + (long long)r0 * e->sstride, e->sstride,
                                              e->n, count, groups, exact32, e->csr_energy.ptr, e->energy + r0, e->stream,
                                              e->shared_j ? e->Rg / e->n_models : 0, e->replica0 + r0));
            return SGA_OK;
        }
        (void)hipGetLastError();  // no room for the transposed spin bits / partial sums: one pass per replica instead
    }
    if (e->groups) {  // group sums from the spin bits, one workgroup per replica (sweep_groups.hip)
        sga::EnergyArgs a{};
        a.h = e->h;
        a.spins = e->spins + (long long)r0 * e->sstride;
        a.energy = e->energy + r0;
        a.n = e->n;
        a.sstride = e->sstride;
        a.R = count;
        a.block_rows = sga::energy_block_rows(e->n);
        a.nblocks = (e->n + a.block_rows - 1) / a.block_rows;
        a.slices = 1;
        HIPCHK(sga::launch_energy_groups(a, e->group_args, e->stream));
        return SGA_OK;
    }
    sga::EnergyArgs a{};
    a.J = e->J_packed;
    a.rowptr = e->rowptr64;
    a.cv = e->cv;
    a.h = e->h;
    a.spins = e->spins + (long long)r0 * e->sstride;
    a.energy = e->energy + r0;
    a.ld = e->ld;
    a.ldj = e->ldj;
    a.n = e->n;
    a.sstride = e->sstride;
    a.R = count;
    a.reps_per_model = e->n_models > 1 ? e->Rg / e->n_models : 0;
    a.replica_base = e->replica0 + r0;
    a.model_stride_j = model_stride_j(e);  // (0: one shared matrix)
    // the canonical order of the sums (sga_kernels.h): blocks of rows (TSP: of cities), a function of n alone
    const int units = e->tsp ? e->tsp_args.n_cities : e->n;
    a.block_rows = e->tsp ? (units + sga::ENERGY_MAX_BLOCKS - 1) / sga::ENERGY_MAX_BLOCKS : sga::energy_block_rows(units);
    a.nblocks = (units + a.block_rows - 1) / a.block_rows;
    // few replicas: spread each replica's blocks over several workgroups (one workgroup reading all
    // of J took 47 ms at n = 10^4 -- longer than the reference's CPU mv)
    // (then as few slices as take the same blocks each, none left without: whole passes of the bit-spin CSR kernel)
    const int per_pass = e->csr && !e->implicit() && sga::energy_csr_bits_form(e->sstride) ? sga::ENERGY_BITS_BLOCKS_PER_PASS : 1;
    const int want = count >= 512 ? 1 : std::max(1, std::min({a.nblocks, (1024 + count - 1) / count, e->n / 8}));
    a.blocks_per_slice = ((a.nblocks + want - 1) / want + per_pass - 1) / per_pass * per_pass;
    a.slices = (a.nblocks + a.blocks_per_slice - 1) / a.blocks_per_slice;
    if (a.slices > 1) {
        const size_t need = sizeof(double) * 2 * (size_t)count * a.nblocks;
        if (need > e->epart_bytes) {
            dev_free(e->epart);
            HIPCHK(hipMalloc(&e->epart, need));
            e->epart_bytes = need;
        }
        a.partial = e->epart;
    }
    HIPCHK(e->tsp ? sga::launch_energy_tsp(a, e->tsp_args, e->stream)
           : e->csr ? sga::launch_energy_csr(a, e->stream)
                    : sga::launch_energy_dense(a, e->want_i8, e->stream));
    HIPCHK(sga::launch_energy_finish(a.partial, a.nblocks, a.slices, a.energy, count, e->stream));
    return SGA_OK;
}

// Launch geometry of the dense kernels for the current replica count / tuning (sga_route.cpp, dense_geometry).  The
// packed matrices are laid out by n alone (pack_dense, at set time), so a change of geometry never touches them.
int ensure_packed(sga_engine *e) {
    if (e->csr || e->implicit()) return SGA_OK;
    if (!e->J_packed) return fail(SGA_ERR_INVALID, "no couplings set");
    const sga_route::DenseGeometry g = sga_route::dense_geometry(route_query_of(e));
    if (e->use_t2 ? (e->ld == g.ld && e->waves_t2 == g.waves_t2 && e->cpw_t2 == g.cpw_t2)
                  : (e->waves == g.waves && e->cpw == g.cpw && e->ld == g.ld))
        return SGA_OK;
    if (!g.fits) return fail(SGA_ERR_UNSUPPORTED, "replica spins do not fit LDS (n too large)");
    if (e->use_t2) {
        e->waves_t2 = g.waves_t2;
        e->cpw_t2 = g.cpw_t2;
    }
    e->waves = g.waves;
    e->cpw = g.cpw;
    e->ld = g.ld;
    return SGA_OK;
}

}  // namespace sga_impl

extern "C" {

const char *sga_last_error(void) { return g_last_error.c_str(); }
// The ABI version, one line per step:
//   3400:    sga_sweep_transverse_dense serves real-valued dense couplings on the fixed-point cached fields of option
//            "clf_fixed_point" (sweep_transverse_fx.hip: D = 2^k J s as exact int32 | int64, any fp32 h; the admission in
//            sga_quantum.h, TrotterProblem::fx_bits); no new entry point, no new option, no engine member
//   3300:    + sga_get_time_links / sga_exchange_transverse: the broken time links of every Trotter group counted on the device
//            (a grid of site chunks x groups, 16-byte loads, one integer atomic per workgroup) and one round of replica
//            exchange between neighbouring groups along the transverse field -- counts, decision, swap of spin rows,
//            energies and valid field rows, bests (trotter_exchange.hip; the admission rules in sga_quantum.h; domain
//            word 8); no option, no engine member
//   3200:    + sga_worldline_clusters_dense: the step of sga_worldline_clusters on dense couplings, decided on the resident
//            fields of every slice -- one workgroup per group, blocks of sites decided in registers, a coupling row read
//            only where a segment flips, the fields kept valid (worldline_clusters_dense.hip; the admission rule in
//            sga_quantum.h); no option, no engine member
//   3100:    + sga_sweep_transverse_dense: the step of sga_sweep_transverse on dense couplings, carried by the cached local
//            fields -- one workgroup per moving slice, a coupling row read on accept only, the fields kept valid
//            (sweep_transverse_clf.hip; the admission rule in sga_kernels.h); no option, no engine member
//   3000:    + sga_worldline_clusters: Swendsen-Wang clusters along imaginary time at one site, flipped under the classical
//            field -- what keeps simulated quantum annealing ergodic at small Gamma; one launch per call, one wave per
//            group of slices, a coupling row read once for all slices of a site (worldline_clusters.hip; the admission
//            rule in sga_kernels.h); domain word 4; no option, no engine member
//   2900:    + sga_sweep_transverse: simulated quantum annealing, the Trotter slices of one instance coupled in the CSR
//            sweep -- two half-sweeps per sweep, the moving slices under h + k (s_up + s_dn) (sweep_transverse.hip; the
//            admission rule in sga_kernels.h); no option, no engine member
//   2800:    + sga_get_class_overlaps / sga_accumulate_ladder_class_overlaps: the overlap between two replicas resolved
//            by a class of sites (planes of a lattice, sublattices, communities), the pairs of two ladders read from the
//            slot map and summed into the caller's first and second moments on the device (class_overlaps.hip; host
//            side in sga_replicas.cpp); read only, no engine state, no option
//   2700:    + sga_get_link_count / sga_get_pair_overlaps / sga_accumulate_ladder_overlaps: spin and link overlaps between
//            pairs of replicas, the pairs of two ladders read from the slot map and histogrammed on the device
//            (pair_overlaps.hip; host side in sga_replicas.cpp); read only, no engine state, no option
//   2600:    + sga_resample: the resampling step of population annealing, planned and copied on the device, exact in
//            integers (resample.hip; host side in sga_replicas.cpp); no engine state, no option
//   2500:    + sga_cluster_move_pairs / sga_cluster_move_ladders: isoenergetic cluster moves between two replicas of one
//            sparse Hamiltonian (cluster_moves.hip; host side in sga_replicas.cpp); no engine state, no option
//   2400:    + sga_set_replica_groups / sga_get_replica_groups: the row-shared sweep over the tile plan runs contiguous
//            groups of replicas as pipelines of their own, a stream each (sweep_dense_rs.hip; " groups=G" behind
//            sga_describe and sga_get_last_kernel where more than one runs); results unchanged
//   2300:    + sga_get_magnetizations / sga_get_overlaps / sga_get_overlaps_with: replica observables as one exact int8
//            product on the matrix cores (observables.hip); read only, no engine state
//   2200:    the row-shared fields in tiles take a plan of their own, sorted by (slice of replicas, tile, replica) in one
//            launch (sweep_dense_rs.hip, rs_tile_plan_kernel); results and interface unchanged
//   2100:    + sga_set_sequential_windows / sga_get_sequential_windows: SGA_SITE_SEQUENTIAL sweeps in windows, the
//            window-start fields of every replica on the matrix cores (sweep_dense_seq.hip; " sweep=seq-windows(W=...)"
//            in sga_describe)
//   2000:    + row-shared windows under SGA_RULE_GLAUBER and SGA_RULE_HEAT_BATH (sweep_dense_rs.hip, ANYRULE;
//            "rule=..." in sga_describe and sga_get_last_kernel), the autotuner's window kept per rule
//   1900:    + options "row_shared_fields", "row_shared_tile_sites": the row-shared fields in tiles of sites, sign-only
//            rows (sweep_dense_rs.hip, rs_fields_tiles_kernel)
//   1800:    + option "row_shared_grid": row-shared windows for dense J on a binary grid under any h
//            (sweep_dense_rs.hip, GRID), sga_route_query.rs_grid
//   1700:    + sga_set_csr_shared (one set of CSR rows, many field vectors)
//   1600:    + sga_set_dense_shared (one coupling matrix, many field vectors), sga_route_query.shared_j
//   1500:    + sga_get_scan_summary; the dense and CSR setters refuse non-finite J / h
//   1400:    + option "batch_fixed_point": fixed-point cached local fields for many-model dense batches
//            (sweep_clf_fx.hip, MODELS)
//   1300:    + options "ragged_field_cache" and "clf_fixed_point" together: fixed-point cached local fields for ragged
//            CSR batches (sweep_clf_csr.hip)
//   1200:    + sga_set_groups_csr (group couplings plus a stored sparse remainder, sweep_groups.hip)
//   1100:    + option "ragged_field_cache" (cached local fields for ragged CSR batches, sweep_clf_csr.hip)
//   1000:    + sga_set_groups (implicit cardinality-group couplings, sweep_groups.hip)
//   900:     + cached local fields for many-model dense batches (sga_set_dense_batch)
//   800:     + option "clf_fixed_point" over dense couplings (sweep_clf_fx.hip)
//   700:     + option "clf_fixed_point" (cached fields of real-valued CSR couplings)
//   600:     + sga_set_csr_batch / sga_get_batch_model (ragged CSR batches)
//   round 5: + sga_explain_route / sga_get_route_query, sga_get_last_kernel, sga_get_autotune_table, ladder-local
//            sga_exchange
int sga_version(void) { return 3400; }

int sga_create(int device, sga_engine **out) {
    if (!out) return fail(SGA_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(SGA_ERR_DEVICE, "no HIP device available (the engine has no CPU fallback)");
    if (device < 0 || device >= count)
        return fail(SGA_ERR_DEVICE, "device index " + std::to_string(device) + " out of range (" +
                                        std::to_string(count) + " visible)");
    HIPCHK(hipSetDevice(device));
    sga_engine *eng = new (std::nothrow) sga_engine();
    if (!eng) return fail(SGA_ERR_MEMORY, "host allocation failed");
    eng->device = device;
    for (int i = 0; i < OPT_COUNT; ++i) {  // the ONE place the library reads the environment
        const OptDef &d = OPT_DEFS[i];
        eng->opt[i] = d.def;
        const char *v = d.env ? std::getenv(d.env) : nullptr;
        if (v) eng->opt[i] = d.env_presence ? d.env_value : std::max(d.lo, std::min(d.hi, (long long)std::atoll(v)));
    }
    eng->caller_csr_ups = eng->opt[OPT_CSR_UPDATES_PER_STEP];
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            eng->cus = cus;
    }
    e = hipStreamCreateWithFlags(&eng->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete eng;
        return fail(SGA_ERR_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    eng->stream = eng->own_stream;
    e = hipMalloc(&eng->d_count, sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&eng->d_flags, 16 * sizeof(int));
    if (e != hipSuccess) {
        dev_free(eng->d_count);
        (void)hipStreamDestroy(eng->own_stream);
        delete eng;
        return fail(SGA_ERR_MEMORY, "hipMalloc failed");
    }
    *out = eng;
    return SGA_OK;
}

void sga_destroy(sga_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    for (auto &p : e->events) {
        (void)hipEventDestroy(p.first);
        (void)hipEventDestroy(p.second);
    }
    e->free_replicas();
    e->free_problem();
    for (auto &sl : e->scratch) sl.release();
    e->point_sites.release();
    e->point_out.release();
    e->csr_energy.release();
    dev_free(e->d_count);
    dev_free(e->d_flags);
    if (e->fork_ev) (void)hipEventDestroy(e->fork_ev);
    if (e->join_ev) (void)hipEventDestroy(e->join_ev);
    if (e->aux_stream) (void)hipStreamDestroy(e->aux_stream);
    if (e->win.run.fork) (void)hipEventDestroy(e->win.run.fork);
    for (int g = 0; g < sga::RS_MAX_GROUPS - 1; ++g) {  // the replica groups' (sga_windows.cpp, ensure_group_run)
        if (e->win.run.join[g]) (void)hipEventDestroy(e->win.run.join[g]);
        if (e->win.run.stream[g]) (void)hipStreamDestroy(e->win.run.stream[g]);
    }
    if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
    delete e;
}

int sga_set_stream(sga_engine *e, void *hip_stream) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->stream = hip_stream ? (hipStream_t)hip_stream : e->own_stream;
    return SGA_OK;
}

int sga_set_option(sga_engine *e, const char *key, int64_t value) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    const int i = find_option(key);
    if (i < 0) return fail(SGA_ERR_INVALID, std::string("unknown option: ") + (key ? key : "(null)"));
    const OptDef &d = OPT_DEFS[i];
    if (value < d.lo || value > d.hi)
        return fail(SGA_ERR_INVALID, std::string("option ") + key + ": value outside [" + std::to_string(d.lo) + ", " +
                                         std::to_string(d.hi) + "]");
    if (e->opt[i] != (long long)value) {
        // where is this value read?  (include/sga.h: [set] | [init] | [sweep])
        if (d.stage == 2 && e->n > 0) e->opt_stale |= 2, e->opt_stale_key = d.key;
        if (d.stage == 1 && e->R > 0) e->opt_stale |= 1, e->opt_stale_key = d.key;
    }
    e->opt[i] = (long long)value;
    if (i == OPT_CSR_UPDATES_PER_STEP) e->caller_csr_ups = (long long)value;  // (the caller's, as opposed to sga_autotune's pick)
    return SGA_OK;
}

int sga_get_option(sga_engine *e, const char *key, int64_t *value) {
    if (!e || !value) return fail(SGA_ERR_INVALID, "NULL argument");
    const int i = find_option(key);
    if (i < 0) return fail(SGA_ERR_INVALID, std::string("unknown option: ") + (key ? key : "(null)"));
    *value = (int64_t)e->opt[i];
    return SGA_OK;
}

int sga_option_name(int index, char *buf, int buflen) {
    if (!buf || buflen <= 0) return fail(SGA_ERR_INVALID, "bad arguments");
    if (index < 0 || index >= OPT_COUNT) return fail(SGA_ERR_INVALID, "no such option");
    std::snprintf(buf, (size_t)buflen, "%s", OPT_DEFS[index].key);
    return SGA_OK;
}

int sga_set_csr_storage(sga_engine *e, int storage) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (storage != SGA_CSR_STORAGE_AUTO && storage != SGA_CSR_STORAGE_F32 && storage != SGA_CSR_STORAGE_PACKED)
        return fail(SGA_ERR_INVALID, "bad CSR storage");
    // (the problem held is one set of rows under many field vectors: refused here, the setting stays; set before such
    //  a problem, sga_init_replicas refuses -- sga_route.cpp, csr_shared_form)
    if (storage == SGA_CSR_STORAGE_PACKED && e->csr && e->shared_j) {
        sga_route_query q = route_query_of(e);
        q.storage = storage;
        return fail(SGA_ERR_UNSUPPORTED, sga_route::csr_shared_form(q).error);
    }
    e->csr_storage = storage;
    return SGA_OK;
}

int sga_set_tuning(sga_engine *e, int waves_per_replica, int sweeps_per_launch) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (waves_per_replica < 0 || waves_per_replica > sga::MAX_WAVES || sweeps_per_launch < 0)
        return fail(SGA_ERR_INVALID, "bad tuning values");
    if (waves_per_replica > 1 && e->csr && e->shared_j) {  // (as sga_set_csr_storage)
        sga_route_query q = route_query_of(e);
        q.tune_waves = waves_per_replica;
        return fail(SGA_ERR_UNSUPPORTED, sga_route::csr_shared_form(q).error);
    }
    e->tune_waves = e->caller_tune_waves = waves_per_replica;
    e->tune_spl = sweeps_per_launch;
    return SGA_OK;
}

int sga_set_field_cache(sga_engine *e, int mode) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (mode != SGA_FIELD_CACHE_OFF && mode != SGA_FIELD_CACHE_ON && mode != SGA_FIELD_CACHE_AUTO)
        return fail(SGA_ERR_INVALID, "bad field-cache mode");
    if (mode == SGA_FIELD_CACHE_ON && e->ragged && e->opt[OPT_RAGGED_FIELD_CACHE] == 0)
        return fail(SGA_ERR_UNSUPPORTED, "cached local fields are not built for ragged CSR batches (AUTO runs the streaming form)");
    if (mode == SGA_FIELD_CACHE_ON && e->csr && e->shared_j) {
        sga_route_query q = route_query_of(e);
        q.field_cache = mode;
        return fail(SGA_ERR_UNSUPPORTED, sga_route::clf_refusal(q));
    }
    if (mode != e->field_cache) {
        // what an earlier mode learnt about these replicas does not carry over: ON runs every replica on the cached-field
        // kernel (AUTO's per-replica routes would leave some on the row kernels for good), a failed allocation under
        // AUTO is retried, the fields are seeded anew
        e->routing.reset();
        e->fields_valid = false;
    }
    e->field_cache = mode;
    return SGA_OK;
}

int sga_set_sequential_windows(sga_engine *e, int W) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (W != 0 && W != 256 && W != 512 && W != 1024)
        return fail(SGA_ERR_INVALID, "sequential windows: W must be 0 (off), 256, 512 or 1024");
    e->win.seq_w = W;
    return SGA_OK;
}

int sga_set_replica_groups(sga_engine *e, int g) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (g != 0 && g != 1 && g != 2 && g != 4)
        return fail(SGA_ERR_INVALID, "replica groups: g must be 0 (the rule's choice), 1, 2 or 4");
    e->win.groups = g;
    return SGA_OK;
}

int sga_get_replica_groups(sga_engine *e, int *g) {
    if (!e || !g) return fail(SGA_ERR_INVALID, "engine or output is NULL");
    *g = e->win.groups;
    return SGA_OK;
}

int sga_get_sequential_windows(sga_engine *e, int *W) {
    if (!e || !W) return fail(SGA_ERR_INVALID, "engine or output is NULL");
    *W = e->win.seq_w;
    return SGA_OK;
}

static int init_replicas_body(sga_engine *e, int R_local, int R_global, int replica0, uint64_t seed,
                              const int8_t *s0);

int sga_init_replicas(sga_engine *e, int R_local, int R_global, int replica0, uint64_t seed,
                      const int8_t *s0) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    // whatever fails in there, the engine is left with NO replicas (R == 0): a later sweep / snapshot /
    // export then reports SGA_ERR_INVALID instead of launching kernels on half-allocated buffers
    const int rc = init_replicas_body(e, R_local, R_global, replica0, seed, s0);
    if (rc != SGA_OK) {
        (void)hipStreamSynchronize(e->stream);
        e->free_replicas();
    }
    return rc;
}

static int init_replicas_body(sga_engine *e, int R_local, int R_global, int replica0, uint64_t seed,
                              const int8_t *s0) {
    if (e->n <= 0) return fail(SGA_ERR_INVALID, "set the couplings before the replicas");
    if (R_local <= 0 || R_global < R_local || replica0 < 0 || replica0 + R_local > R_global)
        return fail(SGA_ERR_INVALID, "bad replica partition");
    if (e->n_models > 1 && R_global % e->n_models != 0)
        return fail(SGA_ERR_INVALID, "R_global must be a multiple of the number of models");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->free_replicas();
    e->opt_stale &= ~1;
    e->R = R_local;
    e->Rg = R_global;
    e->replica0 = replica0;
    e->seed = seed;
    e->sweeps_done = 0;
    e->rounds = 0;
    e->attempted = 0;
    // WHICH form the replicas are laid out for: sga_route.cpp (pure functions of the problem's traits, the replica count,
    // the tuning and the options; tests/test_host_logic.py pins them)
    if (e->groups) {
        const sga_route::GroupsForm f = sga_route::groups_form(route_query_of(e));
        if (f.error) return fail(SGA_ERR_UNSUPPORTED, f.error);
        e->sstride = f.sstride;
        e->waves = f.waves;
        e->cpw = 0;
    } else if (e->tsp) {
        e->sstride = (e->n + 15) / 16 * 16;
        const sga_route::TspForm t = sga_route::tsp_form(e->tsp_args.npad, e->tune_waves);
        e->tsp_waves = t.waves;
        e->tsp_passes = t.passes;
        e->waves = e->tsp_waves;
        e->cpw = 0;
    } else if (!e->csr) {
        int rc = ensure_packed(e);  // geometry depends on the replica count
        if (rc != SGA_OK) return rc;
        e->sstride = (int)e->ld;
    } else {
        const sga_route::CsrForm f = e->ragged ? sga_route::csr_ragged_form(route_query_of(e))
                                               : sga_route::csr_replica_form(route_query_of(e));
        if (f.error) return fail(SGA_ERR_UNSUPPORTED, f.error);
        e->big = f.bits;
        e->big_form = f.big_form;
        e->sstride = f.sstride;
        e->table_m = f.table_m;
        e->waves = f.waves;
        e->cpw = 0;
        if (f.needs_slots) {
            int rc = ensure_slotted(e);
            if (rc != SGA_OK) return rc;
        }
        e->csr_storage_latched = e->csr_storage;
        if (f.wants_packed) {
            int rc = ensure_packed_entries(e);
            if (rc != SGA_OK) return rc;
        }
        if (e->csr_storage == SGA_CSR_STORAGE_PACKED && !(e->big_form == 1 && e->cvp))
            return fail(SGA_ERR_UNSUPPORTED, "packed CSR entries need integer couplings with |J| <= 127, n < 2^24 "
                                             "and the one-replica-per-workgroup bit-spin form");
    }
    const size_t sb = (size_t)R_local * e->sstride;
    HIPCHK(hipMalloc(&e->spins, sb));
    HIPCHK(hipMalloc(&e->best_spins, sb));
    HIPCHK(hipMalloc(&e->energy, sizeof(double) * R_local));
    HIPCHK(hipMalloc(&e->best_energy, sizeof(double) * R_local));
    HIPCHK(hipMalloc(&e->rep_temp, sizeof(double) * R_local));
    HIPCHK(hipMalloc(&e->n_acc, sizeof(unsigned long long) * R_local));
    HIPCHK(hipMemsetAsync(e->n_acc, 0, sizeof(unsigned long long) * R_local, e->stream));
    {
        std::vector<double> ones((size_t)R_local, 1.0);
        HIPCHK(hipMemcpyAsync(e->rep_temp, ones.data(), sizeof(double) * R_local,
                              hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    if (s0) {
        DevIn<int8_t> in;
        int rc = in.init(e->scratch[1], s0, (size_t)R_local * e->n, e->stream);
        if (rc != SGA_OK) return rc;
        HIPCHK(sga::launch_pad_spins(in.ptr, e->n, e->spins, e->sstride, R_local, e->stream));
        if (e->ragged)  // [R][n_max]: what lies past a replica's model is padding
            HIPCHK(sga::launch_mask_spins_ragged(e->spins, e->sstride, R_local, (uint32_t)replica0, e->d_models,
                                                 R_global / e->n_models, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    } else if (e->ragged) {
        HIPCHK(sga::launch_init_spins_ragged(e->spins, e->sstride, R_local, (uint32_t)seed, (uint32_t)(seed >> 32),
                                             (uint32_t)replica0, e->d_models, R_global / e->n_models, e->stream));
    } else {
        HIPCHK(sga::launch_init_spins(e->spins, e->n, e->sstride, R_local, (uint32_t)seed,
                                      (uint32_t)(seed >> 32), (uint32_t)replica0, e->stream));
    }
    int rc = recompute_energy_range(e, 0, R_local);
    if (rc != SGA_OK) return rc;
    HIPCHK(sga::launch_copy_best(e->energy, e->spins, e->best_energy, e->best_spins, e->sstride,
                                 R_local, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return SGA_OK;
}

// Temperatures lie in [0, inf] (include/sga.h): NaN and anything with the sign bit set (-0.0 included) are refused,
// before anything changes.  Host inputs only: a device array is the caller's to check.
static int check_temperatures(const char *call, const double *T, long long count, long long stride = 1) {
    if (is_device_ptr(T)) return SGA_OK;
    for (long long i = 0; i < count; ++i) {
        const double t = T[i * stride];
        if (std::isnan(t) || std::signbit(t)) {
            char msg[160];
            std::snprintf(msg, sizeof(msg), "%s: temperature %g at index %lld is outside [0, inf]", call, t, i);
            return fail(SGA_ERR_INVALID, msg);
        }
    }
    return SGA_OK;
}

int sga_set_temperatures(sga_engine *e, const double *T) {
    if (!e || !T) return fail(SGA_ERR_INVALID, "NULL argument");
    if (e->R <= 0) return fail(SGA_ERR_INVALID, "no replicas");
    int rc = check_temperatures("sga_set_temperatures", T, e->R);
    if (rc != SGA_OK) return rc;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->rep_temp, T, sizeof(double) * e->R, hipMemcpyDefault, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return SGA_OK;
}

int sga_set_ladder(sga_engine *e, const double *slot_temps, int n_ladders) {
    if (!e || !slot_temps) return fail(SGA_ERR_INVALID, "NULL argument");
    if (e->R <= 0) return fail(SGA_ERR_INVALID, "no replicas");
    if (n_ladders <= 0 || e->Rg % n_ladders != 0)
        return fail(SGA_ERR_INVALID, "R_global must be a multiple of n_ladders");
    if (e->ragged && n_ladders % e->n_models != 0)
        return fail(SGA_ERR_INVALID, "ragged CSR batches: n_ladders must be a multiple of the number of models "
                                     "(a ladder lies within one model)");
    int rc = check_temperatures("sga_set_ladder", slot_temps, e->Rg);
    if (rc != SGA_OK) return rc;
    HIPCHK(hipSetDevice(e->device));
    dev_free(e->slot_temps);
    dev_free(e->slot_to_rep);
    dev_free(e->ex_attempts);
    dev_free(e->ex_accepts);
    const size_t Rg = (size_t)e->Rg;
    HIPCHK(hipMalloc(&e->slot_temps, sizeof(double) * Rg));
    HIPCHK(hipMalloc(&e->slot_to_rep, sizeof(int32_t) * Rg));
    HIPCHK(hipMalloc(&e->ex_attempts, sizeof(long long) * Rg));
    HIPCHK(hipMalloc(&e->ex_accepts, sizeof(long long) * Rg));
    HIPCHK(hipMemcpyAsync(e->slot_temps, slot_temps, sizeof(double) * Rg, hipMemcpyDefault,
                          e->stream));
    std::vector<int32_t> ident(Rg);
    for (size_t i = 0; i < Rg; ++i) ident[i] = (int32_t)i;
    HIPCHK(hipMemcpyAsync(e->slot_to_rep, ident.data(), sizeof(int32_t) * Rg, hipMemcpyHostToDevice,
                          e->stream));
    HIPCHK(hipMemsetAsync(e->ex_attempts, 0, sizeof(long long) * Rg, e->stream));
    HIPCHK(hipMemsetAsync(e->ex_accepts, 0, sizeof(long long) * Rg, e->stream));
    // slot i initially holds replica i: local temperatures are the matching slice
    HIPCHK(hipMemcpyAsync(e->rep_temp, e->slot_temps + e->replica0, sizeof(double) * e->R,
                          hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->n_ladders = n_ladders;
    e->rounds = 0;
    return SGA_OK;
}

// ---- the stages of sga_sweep (below): staging, the plan, launch arguments, dispatch, the launches ------------------------
namespace {

// One sga_sweep call as its stages see it: the scalar arguments, and the schedule / replay inputs and trace outputs on
// the device -- borrowed where they live there, staged otherwise.
struct SweepCall {
    int n_sweeps, site_mode, arith;
    int64_t sched_ss, sched_rs;
    DevIn<double> sched;
    DevIn<int32_t> site;
    DevIn<float> u;
    DevOut<double> etrace, dE;
    DevOut<uint8_t> acc;
    int stage(sga_engine *e, const double *sched_, const int32_t *replay_site, const float *replay_u, double *energy_trace,
              uint8_t *accept_trace, double *dE_trace) {
        const size_t R = (size_t)e->R, per = (size_t)n_sweeps * (size_t)e->n;
        hipStream_t st = e->stream;
        int rc = SGA_OK;
        if (sched_)  // the table's extent, from the strides
            rc = sched.init(e->scratch[0], sched_, (size_t)((n_sweeps - 1) * sched_ss + (e->R - 1) * sched_rs + 1), st);
        if (rc == SGA_OK && site_mode == SGA_SITE_REPLAY) rc = site.init(e->scratch[1], replay_site, R * per, st);
        if (rc == SGA_OK && site_mode != SGA_SITE_RANDOM && replay_u) rc = u.init(e->scratch[2], replay_u, R * per, st);
        if (rc == SGA_OK) rc = etrace.init(e->scratch[3], energy_trace, (size_t)n_sweeps * R, st);
        if (rc == SGA_OK) rc = acc.init(e->scratch[4], accept_trace, R * per, st);
        if (rc == SGA_OK) rc = dE.init(e->scratch[5], dE_trace, R * per, st);
        return rc;
    }
    int finish(hipStream_t st) {
        int rc = etrace.flush(st);
        if (rc == SGA_OK) rc = acc.flush(st);
        if (rc == SGA_OK) rc = dE.flush(st);
        // host-side outputs must be complete, and staged host inputs consumed, before returning
        if (rc == SGA_OK && (sched.staged || site.staged || u.staged || etrace.ptr || acc.ptr || dE.ptr)) HIPCHK(hipStreamSynchronize(st));
        return rc;
    }
};

enum class Cached { NONE, CSR, FIXED_POINT, INTEGER, INTEGER_BATCHED };
struct SweepPlan {  // what holds for every launch of a call
    sga_route_query rq;
    sga_route::ClfLooks looks;
    int spl = 1;                // sweeps per launch
    bool exact_mode = false;    // every sweep its own launch, energies from scratch after it
    Cached cached = Cached::NONE;  // the cached-field kernel of the call (NONE: the row-per-proposal kernels for all)
    int cw = 0;                 // ... its waves per replica,
    int n_clf = 0;              // ... the replicas on it,
    bool mixed = false;         // ... and the others beside them on the row kernels, second stream
    int rs_w = 0;               // row-shared window (0: not this form)
    sga::RowSharedTiles rs_tiles{};  // its fields kernel: tiles of S sites (S = 0: one workgroup per site)
    int rs_groups = 1;          // its replica groups, a stream each (1: every launch on the engine's stream)
    sga::SeqWindows seq{};      // sequential windows (W = 0: not this form)
};

// The policy's look at the acceptance counters (sga_route.cpp, look): one read-back and synchronise when a look is due,
// none otherwise.
int look_at_counters(sga_engine *e, const SweepPlan &p) {
    sga_route::LookInput in;
    in.n = e->n;
    in.R = e->R;
    in.attempted = e->attempted;
    in.theta = sga_route::routing_theta(p.rq);
    in.start_cached = !p.looks.is_auto || sga_route::auto_starts_cached(p.rq);
    in.looks = p.looks;
    in.per_replica = e->opt[OPT_REPLICA_ROUTING] != 0 && !e->csr;  // (the CSR row kernels take no replica lists)
    std::vector<int> model_spins;
    if (e->ragged) {
        for (int r = 0; r < e->R; ++r) model_spins.push_back(spins_of(e, r));
        in.spins = model_spins.data();
    }
    std::vector<unsigned long long> now;
    hipError_t he = hipSuccess;
    const bool reseed = sga_route::look(e->routing, in, [&]() -> const unsigned long long * {
        now.resize((size_t)e->R);
        he = hipMemcpyAsync(now.data(), e->n_acc, sizeof(unsigned long long) * e->R, hipMemcpyDeviceToHost, e->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
        return he == hipSuccess ? now.data() : nullptr;
    });
    HIPCHK(he);
    if (reseed) e->fields_valid = false;  // somebody returns from the row kernels: fields are seeded anew
    return SGA_OK;
}

// replica lists on the device ([0, n_clf): cached-field kernel, [R, R + R - n_clf): row kernels), the second
// stream and the two events that fork / join it
int prepare_mixed(sga_engine *e) {
    const int R = e->R;
    if (!e->d_rep_lists) HIPCHK(hipMalloc(&e->d_rep_lists, sizeof(int) * 2 * (size_t)R));
    if (e->routing.dirty) {
        std::vector<int> lists(2 * (size_t)R, 0);
        int ia = 0, ib = 0;
        for (int r = 0; r < R; ++r) {
            if (e->routing.route[(size_t)r] == 0) lists[(size_t)ia++] = r;
            else lists[(size_t)R + (size_t)ib++] = r;
        }
        HIPCHK(hipMemcpyAsync(e->d_rep_lists, lists.data(), sizeof(int) * lists.size(), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        e->routing.dirty = false;
    }
    if (!e->aux_stream) HIPCHK(hipStreamCreateWithFlags(&e->aux_stream, hipStreamNonBlocking));
    if (!e->fork_ev) HIPCHK(hipEventCreateWithFlags(&e->fork_ev, hipEventDisableTiming));
    if (!e->join_ev) HIPCHK(hipEventCreateWithFlags(&e->join_ev, hipEventDisableTiming));
    return SGA_OK;
}

// The arguments of the launch that starts at sweep k0 of the call, as the row-per-proposal kernels take them.
sga::SweepArgs base_args(const sga_engine *e, const SweepCall &c, const SweepPlan &p, int k0) {
    sga::SweepArgs a{};
    a.J = e->J_packed;
    a.rowptr = e->rowptr;
    a.rowptr64 = e->rowptr64;
    a.rowinfo = e->rowinfo;
    a.cvp = (e->big_form == 1 && e->csr_storage_latched != SGA_CSR_STORAGE_F32) ? e->cvp : nullptr;
    a.csr_acc = e->csr_acc;  // (the table form needs its table: set below once table_m is final)
    // head slots per wave that the longest row needs (the wide bit forms are built per count)
    const long long slots = (e->max_row_len + 63) / 64;
    const long long head = (slots + std::max(e->waves, 1) - 1) / std::max(e->waves, 1);
    a.csr_head = (int)std::min<long long>(std::max<long long>(head, 1), 10);
    a.big = e->big_form;
    // (a slotted layout's row extents include the padding to whole 64-entry slots)
    a.csr_row_cap = (e->csr && e->max_row_len <= 256)
                        ? (int)std::max<long long>(e->slotted ? (e->max_row_len + 63) / 64 * 64 : e->max_row_len, 1) : 0;
    a.csr_pair_ahead = csr_updates_per_step(e);
    // (option "look_ahead" = 0: A/B switch and the parity tests' cross-check)
    a.look_ahead = e->opt[OPT_LOOK_AHEAD] != 0 ? 1 : 0;
    a.force_general = e->opt[OPT_FORCE_GENERAL] != 0 ? 1 : 0;
    a.tsp_parallel = (int)e->opt[OPT_TSP_PARALLEL];
    a.cv = e->cv;
    a.h = e->h;
    a.diag = e->diag;
    a.spins = e->spins;
    a.energy = e->energy;
    a.best_energy = e->best_energy;
    a.best_spins = e->best_spins;
    a.n_accepted = e->n_acc;
    a.rep_temp = e->rep_temp;
    a.sched = c.sched.ptr ? c.sched.ptr + (long long)k0 * c.sched_ss : nullptr;
    a.sched_ss = c.sched_ss;
    a.sched_rs = c.sched_rs;
    const long long off = (long long)k0 * e->n;
    a.replay_site = c.site.ptr ? c.site.ptr + off : nullptr;
    a.replay_u = c.u.ptr ? c.u.ptr + off : nullptr;
    a.replay_stride = (long long)c.n_sweeps * e->n;
    a.energy_trace = (c.etrace.ptr && !p.exact_mode) ? c.etrace.ptr + (long long)k0 * e->R : nullptr;
    a.accept_trace = c.acc.ptr ? c.acc.ptr + off : nullptr;
    a.dE_trace = c.dE.ptr ? c.dE.ptr + off : nullptr;
    a.ld = e->ld;
    a.ldj = e->ldj;
    a.n = e->n;
    a.sstride = e->sstride;
    a.R = e->R;
    a.n_sweeps = std::min(p.spl, c.n_sweeps - k0);
    a.site_mode = c.site_mode;
    a.arith = c.arith;
    a.rule = e->rule;
    a.table_m = p.exact_mode ? 0 : e->table_m;
    a.table_scale = e->csr ? e->table_scale : 1;
    a.table_covers = (e->csr && a.table_m > 0 && (double)e->table_scale * (double)e->csr_row_abs_max <= (double)a.table_m) ? 1 : 0;
    if (a.csr_acc == sga::CSR_ACC_F32_TABLE && a.table_m == 0) a.csr_acc = sga::CSR_ACC_F32;
    a.no_best = p.exact_mode ? 1 : 0;
    a.reps_per_model = (e->n_models > 1 || e->ragged) ? e->Rg / e->n_models : 0;
    a.model_stride_j = model_stride_j(e);  // (0: one shared matrix)
    if (e->ragged) a.ragged = e->ragged_at;
    a.seed_lo = (uint32_t)e->seed;
    a.seed_hi = (uint32_t)(e->seed >> 32);
    a.sweep0 = e->sweeps_done + (uint32_t)k0;
    a.replica0 = (uint32_t)e->replica0;
    return a;
}

// ... and as the plan's cached-field form takes them: the resident fields, their width and scale.
sga::SweepArgs cached_args(const sga_engine *e, const SweepPlan &p, sga::SweepArgs a) {
    a.fields = e->fields;
    a.ldf = e->ldf;
    if (p.cached == Cached::CSR) {
        // sparse couplings: D = J s as int16 in LDS, the row's entries read on accept (sweep_clf_csr.hip)
        // (ragged batches: the batch's longest row and largest model choose the waves; a.ragged picks the build)
        a.clf_hq = e->hq;
        a.clf_row_max = (int)std::min<long long>(e->slotted ? (e->max_row_len + 63) / 64 * 64 : e->max_row_len, 1 << 20);
    }
    if (e->clf_fx_bits) {
        // option "clf_fixed_point": D = 2^k J s exactly (CSR: sweep_clf_csr.hip, dense real-valued couplings:
        // sweep_clf_fx.hip); any single-site rule, site mode and arithmetic -- the same chain as the row kernels
        a.field_bits = e->clf_fx_bits;
        a.field_scale = e->clf_fx_k;
        a.table_m = 0;
    } else if (p.cached != Cached::CSR) {
        if (e->clf_scale == 2)  // half-integer fields: dE = q for q <= 2 M, tabulated at twice the resolution
            a.table_m = (int)std::min(2.0 * (double)e->row_abs_max, 2048.0);
        a.field_bits = e->clf_bits;
        a.field_scale = e->clf_scale;
        a.clf_jmax = e->j_abs_max;
        // option "clf_batched": production arguments commit several accepts per round -- every decision of a
        // super-window guessed at once, the guess checked against the few couplings between the accepting sites
        // (sweep_clfb_impl.h); the same chain.  Ahead while the hottest replica accepts more than ~1 % (first sweeps
        // from random spins 2.19 -> 1.72 ms, sweeps 5-25 0.272 -> 0.245), behind after 100 sweeps (0.105 -> 0.112):
        // 2 = by the hottest replica's acceptance (default), 1 = always, 0 = never (profiles/r04_experiments.md 9)
        a.clf_batched = (e->opt[OPT_CLF_BATCHED] == 1 || (p.looks.adaptive && e->routing.hot)) ? 1 : 0;
    }
    return a;
}

// Everything about the call that its launches share.  May refuse the call (Wolff, cached fields ON where they cannot
// be had); under AUTO a failed allocation of the fields leaves the call on the row-per-proposal kernels.
int plan_sweep(sga_engine *e, const SweepCall &c, SweepPlan &p) {
    const int R = e->R;
    p.rq = route_query_of(e);
    // sweeps per launch: aim for ~50 ms of estimated work per launch (sga_route.cpp)
    p.spl = sga_route::sweeps_per_launch(p.rq, c.n_sweeps, e->tune_spl, e->tsp ? e->tsp_args.npad : 0);
    const bool wolff = e->rule == SGA_RULE_WOLFF;
    if (wolff) {
        if (e->ragged) return fail(SGA_ERR_UNSUPPORTED, "the Wolff rule is not implemented for ragged CSR batches");
        if (e->csr && e->shared_j)
            return fail(SGA_ERR_UNSUPPORTED, "shared-coupling CSR batches: the Wolff rule is not implemented for them");
        if (e->tsp) return fail(SGA_ERR_UNSUPPORTED, "the Wolff rule is not implemented for sga_set_tsp problems");
        if (e->groups) return fail(SGA_ERR_UNSUPPORTED, "the Wolff rule is not implemented for sga_set_groups problems");
        if (sga::wolff_lds_bytes(e->n) > 160 * 1024 - 256)
            return fail(SGA_ERR_UNSUPPORTED, "the Wolff rule keeps spins, cluster and queue in LDS: n <= ~31 000");
        if (c.site_mode == SGA_SITE_SEQUENTIAL && !c.u.ptr)
            return fail(SGA_ERR_INVALID, "sequential Wolff sweeps need replay_u (unused values are fine)");
        // the cluster growth treats every stored entry as one bond: duplicate columns of a row (which the
        // other rules add up) would be drawn twice and could overrun the cluster queue
        if (e->csr && !e->csr_sorted)
            return fail(SGA_ERR_UNSUPPORTED, "the Wolff rule over CSR couplings needs rows strictly sorted by "
                                             "column (no duplicate entries)");
    }
    // Asymmetric J or a non-zero diagonal: the rule's dE (row i only, as the reference computes
    // it) is not the energy change, so E += dE would drift from compute_energy().  Then every
    // sweep is its own launch, followed by a from-scratch energy evaluation and the best update
    // (exactly the reference's sequence, core/spin_dynamics.py:87, gpu_annealer.py:151-153).
    // (the Wolff rule reports compute_energy() after every sweep as well, spin_dynamics.py:87)
    p.exact_mode = !e->consistent_dE || wolff;
    if (p.exact_mode) p.spl = 1;
    // cached local fields (sga_set_field_cache): a row is read only when a proposal is accepted
    bool clf = false;
    if (e->field_cache != SGA_FIELD_CACHE_OFF && !wolff) {
        const char *why = nullptr;
        clf = clf_possible(e, &why);
        if (!clf && e->field_cache == SGA_FIELD_CACHE_ON) return fail(SGA_ERR_UNSUPPORTED, why);
    }
    p.n_clf = clf ? R : 0;
    if (clf) p.looks = sga_route::clf_looks(p.rq);
    if (p.looks.any()) {  // (unavailable, below, is only ever set under AUTO)
        int rc = e->routing.unavailable ? SGA_OK : look_at_counters(e, p);
        if (rc != SGA_OK) return rc;
        p.n_clf = e->routing.unavailable ? 0 : e->routing.n_cached;
        clf = p.n_clf > 0;
    }
    if (clf) {
        int rc = ensure_fields(e);
        if (rc == SGA_ERR_MEMORY && e->field_cache == SGA_FIELD_CACHE_AUTO) {
            // AUTO promises a faster form where it is available, not a failure where the row-per-proposal kernels
            // (which need none of this memory) would have run: the cache is "not available" for these replicas
            e->routing.unavailable = true;
            dev_free(e->fields);
            clf = false;
            p.n_clf = 0;
        } else if (rc != SGA_OK) {
            return rc;
        }
    }
    p.mixed = clf && p.n_clf < R;  // some replicas of this call on the row-per-proposal kernels beside the cached ones
    if (p.mixed) {
        int rc = prepare_mixed(e);
        if (rc != SGA_OK) return rc;
    }
    if (!clf) e->fields_valid = false;  // the row-per-proposal kernels move the spins only
    if (clf) {
        // no row streaming to bound the launch by: many sweeps per launch (a sweep is 0.1 ... 10 ms here:
        // at most 256 of them, so that a launch stays well under a few seconds)
        if (!p.mixed && e->tune_spl <= 0) p.spl = std::min(c.n_sweeps, 256);
        p.cached = e->csr ? Cached::CSR : e->clf_fx_bits ? Cached::FIXED_POINT : Cached::INTEGER;
        p.cw = e->csr ? sga_route::clf_csr_waves(p.rq)
               : (p.looks.tail && e->routing.wide)
                   ? 8
                   : sga::sweep_clf_waves(e->ldj, e->want_i8, p.mixed ? p.n_clf : R, e->cus, (int)e->opt[OPT_CLF_WAVES]);
        // Whether the batched / the CSR form applies is asked once, of the first launch's arguments: it depends on which
        // pointers are set, the modes and the sizes, and those are the same for every launch of a call.
        const sga::SweepArgs ac = cached_args(e, p, base_args(e, c, p, 0));
        if (p.cached == Cached::INTEGER && sga::sweep_clfb_applies(ac, e->want_i8)) p.cached = Cached::INTEGER_BATCHED;
        // CSR: production arguments only -- traced / replayed / sequential sweeps take the row-per-proposal kernels
        // (the same chain) and the fields are seeded anew afterwards
        if (p.cached == Cached::CSR && !sga::sweep_clf_csr_applies(ac, p.cw)) {
            p.cached = Cached::NONE;
            e->fields_valid = false;
        }
    }
    // the window forms (sga_windows.cpp): row-shared windows for production arguments, sequential windows for sequential
    // sweeps, neither with per-update traces; a form whose scratch cannot be had leaves the row-per-proposal kernel
    if (!clf && !p.exact_mode) {  // (exact_mode: the Wolff rule too)
        const bool untraced = !c.acc.ptr && !c.dE.ptr;
        plan_windows(e, untraced && c.site_mode == SGA_SITE_RANDOM && c.arith == SGA_ARITH_F64,
                     untraced && c.site_mode == SGA_SITE_SEQUENTIAL, c.etrace.ptr != nullptr, p.rs_w, p.rs_tiles, p.rs_groups, p.seq);
    }
    return SGA_OK;
}

// the row-per-proposal kernel of a dense problem (all replicas, or the list in a.rep_list)
hipError_t launch_dense_rows(const sga_engine *e, sga::SweepArgs a, hipStream_t st) {
    const bool lean = !a.force_general && a.site_mode == SGA_SITE_RANDOM && a.arith == SGA_ARITH_F64 &&
                      e->rule == SGA_RULE_METROPOLIS && !a.accept_trace && !a.dE_trace;
    if (e->use_t2 && lean) {  // production sweeps read the two bit-planes
        a.J = e->J_bits;
        a.J_aux = e->J_packed;
        a.plane_row_bytes = t2_row_bits(e->n) / 8;
        a.plane_bytes = (long long)e->n * a.plane_row_bytes;
        a.diag = e->row_nnz;
        return sga::launch_sweep_dense_t2(a, e->waves_t2, e->cpw_t2 > sga::T2_MAX_CPW ? 0 : e->cpw_t2, st);
    }
    return sga::launch_sweep_dense(a, e->want_i8, e->acc64 ? (e->acc_canon ? 2 : 1) : 0, e->waves,
                                   e->cpw > sga::MAX_CPW ? 0 : e->cpw, st);
}

hipError_t launch_cached(const sga_engine *e, const SweepPlan &p, const sga::SweepArgs &ac, hipStream_t st) {
    if (p.cached == Cached::CSR) return sga::launch_sweep_clf_csr(ac, p.cw, st);
    if (p.cached == Cached::FIXED_POINT) return sga::launch_sweep_clf_fx(ac, e->want_i8, p.cw, st, e->n_models);
    if (p.cached == Cached::INTEGER_BATCHED) return sga::launch_sweep_clfb(ac, e->want_i8, p.cw, st);
    return sga::launch_sweep_clf(ac, e->want_i8, p.cw, st);
}

// Two launches over disjoint replica lists, side by side: the cached-field kernel on the engine's stream, the
// row-per-proposal kernel on the second one, forked and joined by events.
hipError_t launch_mixed(sga_engine *e, const SweepPlan &p, sga::SweepArgs ac, sga::SweepArgs a, hipStream_t st) {
    ac.rep_list = e->d_rep_lists;
    ac.rep_count = p.n_clf;
    a.rep_list = e->d_rep_lists + e->R;
    a.rep_count = e->R - p.n_clf;
    hipError_t le = hipEventRecord(e->fork_ev, st);
    if (le == hipSuccess) le = hipStreamWaitEvent(e->aux_stream, e->fork_ev, 0);
    if (le == hipSuccess) le = launch_cached(e, p, ac, st);
    char first[200], both[448];
    std::snprintf(first, sizeof(first), "%s", sga::last_sweep_kernel());
    if (le == hipSuccess) le = launch_dense_rows(e, a, e->aux_stream);
    if (le == hipSuccess) le = hipEventRecord(e->join_ev, e->aux_stream);
    if (le == hipSuccess) le = hipStreamWaitEvent(st, e->join_ev, 0);
    if (le != hipSuccess) (void)hipStreamSynchronize(e->aux_stream);
    std::snprintf(both, sizeof(both), "mixed launch: %d replica(s) on %s || %d on %s", p.n_clf, first, e->R - p.n_clf,
                  sga::last_sweep_kernel());
    sga::note_sweep_kernel("%s", both);
    return le;
}

// One launch of the plan's form: cached fields, else the rule's / the problem's own kernel.
hipError_t launch_sweep(sga_engine *e, const SweepPlan &p, sga::SweepArgs a, hipStream_t st) {
    if (p.cached != Cached::NONE) {
        const sga::SweepArgs ac = cached_args(e, p, a);
        return p.mixed ? launch_mixed(e, p, ac, a, st) : launch_cached(e, p, ac, st);
    }
    if (e->rule == SGA_RULE_WOLFF) return sga::launch_sweep_wolff(a, sga::WolffArgs{e->wolff_u, e->wolff_cap, e->wolff_cursor}, e->csr, e->want_i8, st);
    if (e->implicit()) a.table_m = 0;
    if (e->groups) return sga::launch_sweep_groups(a, e->group_args, e->waves, st);
    if (e->tsp) return sga::launch_sweep_tsp(a, e->tsp_args, e->tsp_waves, e->tsp_passes, st);
    if (e->csr) return sga::launch_sweep_csr(a, e->waves, st);
    if (p.seq.W) return sga::launch_sweep_dense_seq(a, p.seq, e->want_i8, e->cus, st);
    if (p.rs_w) {
        e->win.run.G = p.rs_groups;
        return sga::launch_sweep_dense_rs(a, e->win.rs, e->want_i8, st, e->win.rs_grid, p.rs_tiles, p.rs_groups > 1 ? &e->win.run : nullptr);
    }
    return launch_dense_rows(e, a, st);
}

// The call's launches, spl sweeps each; exact_mode: energies from scratch and the best update after every one.
int run_launches(sga_engine *e, const SweepCall &c, const SweepPlan &p) {
    const int R = e->R;
    hipStream_t st = e->stream;
    for (int k0 = 0; k0 < c.n_sweeps; k0 += p.spl) {
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        if (e->timing) {
            HIPCHK(hipEventCreate(&ev0));
            const hipError_t ce = hipEventCreate(&ev1);
            if (ce != hipSuccess) {
                (void)hipEventDestroy(ev0);
                HIPCHK(ce);
            }
            HIPCHK(hipEventRecord(ev0, st));
        }
        const hipError_t le = launch_sweep(e, p, base_args(e, c, p, k0), st);
        if (e->timing) {
            (void)hipEventRecord(ev1, st);
            e->events.emplace_back(ev0, ev1);
        }
        if (le != hipSuccess) (void)hipStreamSynchronize(st);  // staged inputs / scratch slots are reusable again
        HIPCHK(le);
        std::snprintf(e->last_kernel, sizeof(e->last_kernel), "%s", sga::last_sweep_kernel());  // (this thread just launched it)
        if (p.exact_mode) {
            int rc = recompute_energy_range(e, 0, R);
            if (rc != SGA_OK) return rc;
            HIPCHK(sga::launch_update_best(e->energy, e->spins, e->best_energy, e->best_spins, e->sstride, R, st));
            if (c.etrace.ptr)
                HIPCHK(hipMemcpyAsync(c.etrace.ptr + (long long)k0 * R, e->energy, sizeof(double) * R, hipMemcpyDeviceToDevice, st));
        }
    }
    return SGA_OK;
}

}  // namespace

int sga_sweep(sga_engine *e, int n_sweeps, int site_mode, int arith, const double *sched,
              int64_t sched_sweep_stride, int64_t sched_replica_stride,
              const int32_t *replay_site, const float *replay_u, double *energy_trace,
              uint8_t *accept_trace, double *dE_trace) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (e->R <= 0) return fail(SGA_ERR_INVALID, "no replicas (call sga_init_replicas)");
    if (n_sweeps < 0) return fail(SGA_ERR_INVALID, "n_sweeps < 0");
    if (site_mode < SGA_SITE_RANDOM || site_mode > SGA_SITE_REPLAY)
        return fail(SGA_ERR_INVALID, "bad site_mode");
    if (arith != SGA_ARITH_F64 && arith != SGA_ARITH_F32) return fail(SGA_ERR_INVALID, "bad arith");
    if (e->rule != SGA_RULE_METROPOLIS && arith != SGA_ARITH_F64)
        return fail(SGA_ERR_INVALID, "Glauber / heat-bath rules need SGA_ARITH_F64");
    if (site_mode == SGA_SITE_REPLAY && (!replay_site || !replay_u))
        return fail(SGA_ERR_INVALID, "SITE_REPLAY needs replay_site and replay_u");
    if (n_sweeps == 0) return SGA_OK;
    if (sched && (sched_sweep_stride < 0 || sched_replica_stride < 0)) return fail(SGA_ERR_INVALID, "negative schedule stride");
    if (sched && !is_device_ptr(sched)) {  // every T(k, r) this call reads, before the first piece runs
        for (int r = 0; r < e->R; ++r) {
            int rc = check_temperatures("sga_sweep (sched)", sched + (long long)r * sched_replica_stride, n_sweeps,
                                        sched_sweep_stride);
            if (rc != SGA_OK) return rc;
        }
    }
    if (e->opt_stale)
        return fail(SGA_ERR_INVALID, std::string("option \"") + (e->opt_stale_key ? e->opt_stale_key : "?") + "\" changed after " +
                                         ((e->opt_stale & 2) ? "the couplings were set (it is read by sga_set_dense / sga_set_csr): set them again"
                                                             : "sga_init_replicas (it is read there): initialise the replicas again"));
    HIPCHK(hipSetDevice(e->device));
    int rc = ensure_packed(e);
    if (rc != SGA_OK) return rc;
    if (!e->csr && !e->implicit() && e->sstride != (int)e->ld)
        return fail(SGA_ERR_INVALID, "tuning changed after sga_init_replicas; re-initialise");
    // The cached-field modes pick their kernel form by the acceptance counters, looked at when a call starts: a long
    // production call is walked in pieces of 16 sweeps so that the form follows the run (the chain does not depend on
    // how a run is cut into calls).  Only where the counters ARE looked at: AUTO, and ON over dense couplings with the
    // tail / batched forms enabled -- ON over CSR couplings has one form: its call stays one piece, launches of up to
    // 256 sweeps.
    constexpr int PIECE = 16;
    if (n_sweeps > PIECE && e->field_cache != SGA_FIELD_CACHE_OFF && e->rule != SGA_RULE_WOLFF && site_mode == SGA_SITE_RANDOM &&
        !replay_site && !replay_u && !accept_trace && !dE_trace &&
        sga_route::clf_looks(route_query_of(e), false).any() && clf_possible(e, nullptr)) {
        for (int k = 0; k < n_sweeps && rc == SGA_OK; k += PIECE)
            rc = sga_sweep(e, std::min(PIECE, n_sweeps - k), site_mode, arith, sched ? sched + (long long)k * sched_sweep_stride : nullptr,
                           sched_sweep_stride, sched_replica_stride, nullptr, nullptr,
                           energy_trace ? energy_trace + (size_t)k * (size_t)e->R : nullptr, nullptr, nullptr);
        return rc;
    }
    SweepCall c{n_sweeps, site_mode, arith, sched_sweep_stride, sched_replica_stride};
    rc = c.stage(e, sched, replay_site, replay_u, energy_trace, accept_trace, dE_trace);
    SweepPlan p;
    if (rc == SGA_OK) rc = plan_sweep(e, c, p);
    if (rc == SGA_OK) rc = run_launches(e, c, p);
    if (rc != SGA_OK) return rc;
    e->sweeps_done += (uint32_t)n_sweeps;
    e->attempted += (long long)n_sweeps * e->n;
    return c.finish(e->stream);
}

int sga_set_update_rule(sga_engine *e, int rule) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (rule < SGA_RULE_METROPOLIS || rule > SGA_RULE_WOLFF)
        return fail(SGA_ERR_UNSUPPORTED, "update rule not implemented by the engine");
    if (rule == SGA_RULE_WOLFF && e->tsp)
        return fail(SGA_ERR_UNSUPPORTED, "the Wolff rule is not implemented for sga_set_tsp problems");
    if (rule == SGA_RULE_WOLFF && e->groups)
        return fail(SGA_ERR_UNSUPPORTED, "the Wolff rule is not implemented for sga_set_groups problems");
    if (rule == SGA_RULE_WOLFF && e->ragged)
        return fail(SGA_ERR_UNSUPPORTED, "the Wolff rule is not implemented for ragged CSR batches");
    if (rule == SGA_RULE_WOLFF && e->csr && e->shared_j)
        return fail(SGA_ERR_UNSUPPORTED, "shared-coupling CSR batches: the Wolff rule is not implemented for them");
    e->rule = rule;
    return SGA_OK;
}

int sga_set_wolff_replay(sga_engine *e, const float *u, int64_t capacity) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (e->R <= 0) return fail(SGA_ERR_INVALID, "no replicas");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    dev_free(e->wolff_u);
    dev_free(e->wolff_cursor);
    e->wolff_cap = 0;
    if (!u || capacity <= 0) return SGA_OK;
    HIPCHK(hipMalloc(&e->wolff_u, sizeof(float) * (size_t)e->R * (size_t)capacity));
    HIPCHK(hipMalloc(&e->wolff_cursor, sizeof(long long) * (size_t)e->R));
    HIPCHK(hipMemcpy(e->wolff_u, u, sizeof(float) * (size_t)e->R * (size_t)capacity, hipMemcpyDefault));
    HIPCHK(hipMemset(e->wolff_cursor, 0, sizeof(long long) * (size_t)e->R));
    e->wolff_cap = capacity;
    return SGA_OK;
}

int sga_recompute_energies(sga_engine *e) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (e->R <= 0) return fail(SGA_ERR_INVALID, "no replicas");
    HIPCHK(hipSetDevice(e->device));
    return recompute_energy_range(e, 0, e->R);
}

static int point_op(sga_engine *e, int r, const int32_t *sites, int count, int op, double T,
                    float u, int arith, double *out_host, int out_count) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (e->R <= 0 || r < 0 || r >= e->R) return fail(SGA_ERR_INVALID, "bad replica index");
    if (!sites || count <= 0) return fail(SGA_ERR_INVALID, "no sites");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    std::vector<int32_t> hs((size_t)count);
    if (is_device_ptr(sites))
        HIPCHK(hipMemcpy(hs.data(), sites, sizeof(int32_t) * hs.size(), hipMemcpyDeviceToHost));
    else
        std::memcpy(hs.data(), sites, sizeof(int32_t) * hs.size());
    if (e->ragged && op != 0)
        return fail(SGA_ERR_UNSUPPORTED, "single-site flip / update are not implemented for ragged CSR batches "
                                         "(sga_sweep and sga_local_fields are)");
    const int n_r = spins_of(e, r);
    for (int32_t v : hs)
        if (v < 0 || v >= n_r) return fail(SGA_ERR_INVALID, "site index out of range");
    if (op == 2 && e->rule == SGA_RULE_WOLFF)
        return fail(SGA_ERR_UNSUPPORTED, "sga_update applies single-site rules; Wolff moves run through sga_sweep");
    if (e->implicit()) {  // structured couplings: local fields only (flip / update go through sweeps)
        if (op != 0)
            return fail(SGA_ERR_UNSUPPORTED, e->groups ? "single-site flip / update are not implemented for sga_set_groups problems"
                                                       : "single-site flip / update are not implemented for sga_set_tsp problems");
        HIPCHK(e->point_sites.reserve(sizeof(int32_t) * hs.size()));
        HIPCHK(e->point_out.reserve(sizeof(double) * (size_t)out_count));
        HIPCHK(hipMemcpyAsync(e->point_sites.ptr, hs.data(), sizeof(int32_t) * hs.size(), hipMemcpyHostToDevice, st));
        if (e->groups)
            HIPCHK(sga::launch_fields_groups(e->group_args, e->spins + (long long)r * e->sstride, e->h,
                                             static_cast<const int32_t *>(e->point_sites.ptr), count,
                                             static_cast<double *>(e->point_out.ptr), st));
        else
            HIPCHK(sga::launch_fields_tsp(e->tsp_args, e->spins + (long long)r * e->sstride, e->h,
                                          static_cast<const int32_t *>(e->point_sites.ptr), count,
                                          static_cast<double *>(e->point_out.ptr), st));
        HIPCHK(hipMemcpyAsync(out_host, e->point_out.ptr, sizeof(double) * (size_t)out_count, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return SGA_OK;
    }
    // staging in grow-only scratch slots (no allocation / free per call)
    HIPCHK(e->point_sites.reserve(sizeof(int32_t) * hs.size()));
    HIPCHK(e->point_out.reserve(sizeof(double) * (size_t)std::max(out_count, 2)));
    int32_t *d_sites = static_cast<int32_t *>(e->point_sites.ptr);
    double *d_out = static_cast<double *>(e->point_out.ptr);
    hipError_t he = hipMemcpyAsync(d_sites, hs.data(), sizeof(int32_t) * hs.size(), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) {
        sga::PointArgs a{};
        const long long model = e->n_models > 1 ? (e->replica0 + r) / (e->Rg / e->n_models) : 0;
        a.J = e->J_packed;
        a.model_offset_j = model * model_stride_j(e);  // (one shared matrix: 0; h and diag are per model)
        a.rowptr = e->rowptr64;
        a.cv = e->cv;
        a.h = e->h + model * e->n;
        a.diag = e->diag + (e->csr ? 0 : model * e->n);  // (sga_set_csr_shared: the diagonal is J's, held once)
        if (e->ragged) {  // the model's rows (its columns are model-local)
            const int row0 = e->model_row0[(size_t)model_of(e, r)];
            a.model_offset_j = 0;
            a.rowptr = e->rowptr64 + row0;
            a.h = e->h + row0;
            a.diag = e->diag + row0;
        }
        a.spins = e->spins + (long long)r * e->sstride;
        a.energy = e->energy + r;
        a.n_accepted = e->n_acc + r;
        a.sites = d_sites;
        a.out = d_out;
        a.ld = e->ld;
        a.ldj = e->ldj;
        a.n = n_r;
        a.count = count;
        a.op = op;
        a.arith = arith;
        a.rule = e->rule;
        a.T = T;
        a.u = u;
        he = sga::launch_point_op(a, e->csr, e->want_i8, st);
    }
    if (he == hipSuccess)
        he = hipMemcpyAsync(out_host, d_out, sizeof(double) * (size_t)out_count, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    HIPCHK(he);
    if (op != 0) e->fields_valid = false;
    if (op != 0 && !e->consistent_dE) {  // the rule's dE is not the energy change here
        int rc = recompute_energy_range(e, r, 1);
        if (rc != SGA_OK) return rc;
        HIPCHK(hipStreamSynchronize(st));
    }
    return SGA_OK;
}

int sga_local_fields(sga_engine *e, int r, const int32_t *sites, int count, double *out) {
    if (!out) return fail(SGA_ERR_INVALID, "out is NULL");
    if (is_device_ptr(out)) return fail(SGA_ERR_INVALID, "out must be a host buffer");
    return point_op(e, r, sites, count, 0, 1.0, 0.0f, SGA_ARITH_F64, out, count);
}

int sga_flip(sga_engine *e, int r, int site, double *dE) {
    double o[2] = {0.0, 0.0};
    const int32_t s = site;
    int rc = point_op(e, r, &s, 1, 1, 1.0, 0.0f, SGA_ARITH_F64, o, 2);
    if (rc == SGA_OK && dE) *dE = o[0];
    return rc;
}

int sga_update(sga_engine *e, int r, int site, double T, float u, int arith, int *accepted,
               double *dE) {
    if (arith != SGA_ARITH_F64 && arith != SGA_ARITH_F32) return fail(SGA_ERR_INVALID, "bad arith");
    double o[2] = {0.0, 0.0};
    const int32_t s = site;
    int rc = point_op(e, r, &s, 1, 2, T, u, arith, o, 2);
    if (rc == SGA_OK) {
        if (accepted) *accepted = o[1] != 0.0;
        if (dE) *dE = o[0];
    }
    return rc;
}

int sga_exchange(sga_engine *e, const double *energies_global, const int32_t *start,
                 const double *u, int *n_accepted) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (e->n_ladders <= 0) return fail(SGA_ERR_INVALID, "no ladder (call sga_set_ladder)");
    const int L = e->Rg / e->n_ladders;
    // whole ladders on this rank: their rounds need nobody else's energies (zero exchange traffic)
    const bool ladders_local = !energies_global && e->R != e->Rg && e->replica0 % L == 0 && e->R % L == 0;
    if (!energies_global && e->R != e->Rg && !ladders_local)
        return fail(SGA_ERR_INVALID, "sharded replicas need the all-gathered energies (unless every ladder lies "
                                     "whole on one rank)");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    DevIn<double> d_e, d_u;
    DevIn<int32_t> d_start;
    int rc;
    if (energies_global) {
        rc = d_e.init(e->scratch[6], energies_global, (size_t)e->Rg, st);
        if (rc != SGA_OK) return rc;
    }
    if (start) {
        rc = d_start.init(e->scratch[7], start, (size_t)e->n_ladders, st);
        if (rc != SGA_OK) return rc;
    }
    if (u) {
        rc = d_u.init(e->scratch[8], u, (size_t)e->n_ladders * (L / 2), st);
        if (rc != SGA_OK) return rc;
    }
    HIPCHK(hipMemsetAsync(e->d_count, 0, sizeof(int), st));
    sga::ExchangeArgs a{};
    a.energies = energies_global ? d_e.ptr : e->energy;
    a.slot_temps = e->slot_temps;
    a.slot_to_rep = e->slot_to_rep;
    a.rep_temp = e->rep_temp;
    a.attempts = e->ex_attempts;
    a.accepts = e->ex_accepts;
    a.start = d_start.ptr;
    a.u = d_u.ptr;
    a.n_accepted = e->d_count;
    a.R_global = e->Rg;
    a.R_local = e->R;
    a.replica0 = e->replica0;
    a.n_ladders = e->n_ladders;
    a.seed_lo = (uint32_t)e->seed;
    a.seed_hi = (uint32_t)(e->seed >> 32);
    a.round = e->rounds;
    a.ladder0 = ladders_local ? e->replica0 / L : 0;
    a.n_ladders_local = ladders_local ? e->R / L : e->n_ladders;
    a.energy_base = ladders_local ? e->replica0 : 0;
    HIPCHK(sga::launch_exchange_neighbor(a, st));
    e->rounds += 1;
    if (n_accepted) {
        HIPCHK(hipMemcpyAsync(n_accepted, e->d_count, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    } else if (d_e.staged || d_u.staged || d_start.staged) {
        HIPCHK(hipStreamSynchronize(st));  // the host buffers may be reused by the caller
    }
    return SGA_OK;
}

int sga_exchange_pairs(sga_engine *e, const double *energies_global, const int32_t *pairs,
                       const double *u, int count, int *n_accepted) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (e->n_ladders <= 0) return fail(SGA_ERR_INVALID, "no ladder (call sga_set_ladder)");
    if (!energies_global && e->R != e->Rg)
        return fail(SGA_ERR_INVALID, "sharded replicas need the all-gathered energies");
    if (count < 0 || (count > 0 && !pairs)) return fail(SGA_ERR_INVALID, "bad pair list");
    if (is_device_ptr(pairs)) return fail(SGA_ERR_INVALID, "pairs must be a host buffer");
    for (int k = 0; k < 2 * count; ++k)
        if (pairs[k] < 0 || pairs[k] >= e->Rg) return fail(SGA_ERR_INVALID, "slot index out of range");
    if (e->ragged) {  // slots of a ladder hold replicas of its model only: a pair across two models is refused
        const int reps = e->Rg / e->n_models;
        for (int k = 0; k < count; ++k)
            if (pairs[2 * k] / reps != pairs[2 * k + 1] / reps)
                return fail(SGA_ERR_INVALID, "ragged CSR batch: pair " + std::to_string(k) + " joins slots of models " +
                                                 std::to_string(pairs[2 * k] / reps) + " and " +
                                                 std::to_string(pairs[2 * k + 1] / reps));
    }
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    DevIn<double> d_e, d_u;
    DevIn<int32_t> d_pairs;
    int rc;
    if (energies_global) {
        rc = d_e.init(e->scratch[6], energies_global, (size_t)e->Rg, st);
        if (rc != SGA_OK) return rc;
    }
    rc = d_pairs.init(e->scratch[7], pairs, (size_t)2 * count, st);
    if (rc != SGA_OK) return rc;
    if (u) {
        rc = d_u.init(e->scratch[8], u, (size_t)count, st);
        if (rc != SGA_OK) return rc;
    }
    sga::ExchangeArgs a{};
    a.energies = energies_global ? d_e.ptr : e->energy;
    a.slot_temps = e->slot_temps;
    a.slot_to_rep = e->slot_to_rep;
    a.rep_temp = e->rep_temp;
    a.attempts = e->ex_attempts;
    a.accepts = e->ex_accepts;
    a.u = d_u.ptr;
    a.n_accepted = e->d_count;
    a.R_global = e->Rg;
    a.R_local = e->R;
    a.replica0 = e->replica0;
    a.n_ladders = e->n_ladders;
    a.seed_lo = (uint32_t)e->seed;
    a.seed_hi = (uint32_t)(e->seed >> 32);
    a.round = e->rounds;
    HIPCHK(sga::launch_exchange_pairs(a, d_pairs.ptr, count, st));
    e->rounds += 1;
    int cnt = 0;  // (the pair list was staged from the host: synchronise in any case)
    HIPCHK(hipMemcpyAsync(&cnt, e->d_count, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_accepted) *n_accepted = cnt;
    return SGA_OK;
}

int sga_op_pt_exchange(int device, float *spins, float *energies, const float *temps,
                       const float *u, uint64_t seed, uint32_t round, int R, int n,
                       int *n_accepted) {
    if (!spins || !energies || !temps || R <= 0 || n <= 0)
        return fail(SGA_ERR_INVALID, "bad operator-exchange arguments");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count)
        return fail(SGA_ERR_DEVICE, "no such HIP device");
    HIPCHK(hipSetDevice(device));
    hipStream_t st = nullptr;  // default stream: ordered with the caller's legacy-stream work
    const size_t rows = (size_t)R * n;
    float *d_spins = nullptr, *d_tmp = nullptr, *d_en = nullptr;
    int32_t *d_src = nullptr;
    int *d_cnt = nullptr;
    DevIn<float> d_t, d_uu;
    Scratch tmp_t, tmp_u;  // stateless entry point: its own short-lived staging
    struct Release {
        Scratch &a, &b;
        ~Release() { a.release(); b.release(); }
    } release_on_exit{tmp_t, tmp_u};
    int rc = d_t.init(tmp_t, temps, (size_t)R, st);
    if (rc != SGA_OK) return rc;
    if (u && R > 1) {
        rc = d_uu.init(tmp_u, u, (size_t)(R - 1), st);
        if (rc != SGA_OK) return rc;
    }
    const bool spins_dev = is_device_ptr(spins), en_dev = is_device_ptr(energies);
    auto cleanup = [&]() {
        if (!spins_dev) dev_free(d_spins);
        if (!en_dev) dev_free(d_en);
        dev_free(d_tmp);
        dev_free(d_src);
        dev_free(d_cnt);
    };
    hipError_t he = hipSuccess;
    auto step = [&](hipError_t x) {
        if (he == hipSuccess) he = x;
    };
    if (spins_dev) d_spins = spins; else step(hipMalloc(&d_spins, rows * sizeof(float)));
    if (en_dev) d_en = energies; else step(hipMalloc(&d_en, (size_t)R * sizeof(float)));
    step(hipMalloc(&d_tmp, rows * sizeof(float)));
    step(hipMalloc(&d_src, (size_t)R * sizeof(int32_t)));
    step(hipMalloc(&d_cnt, sizeof(int)));
    if (he == hipSuccess && !spins_dev)
        step(hipMemcpyAsync(d_spins, spins, rows * sizeof(float), hipMemcpyHostToDevice, st));
    if (he == hipSuccess && !en_dev)
        step(hipMemcpyAsync(d_en, energies, (size_t)R * sizeof(float), hipMemcpyHostToDevice, st));
    if (he == hipSuccess)
        step(sga::launch_op_exchange(d_spins, d_tmp, d_en, d_t.ptr, d_uu.ptr, d_src, d_cnt,
                                     (uint32_t)seed, (uint32_t)(seed >> 32), round, R, n, st));
    if (he == hipSuccess && !spins_dev)
        step(hipMemcpyAsync(spins, d_spins, rows * sizeof(float), hipMemcpyDeviceToHost, st));
    if (he == hipSuccess && !en_dev)
        step(hipMemcpyAsync(energies, d_en, (size_t)R * sizeof(float), hipMemcpyDeviceToHost, st));
    int cnt = 0;
    if (he == hipSuccess) step(hipMemcpyAsync(&cnt, d_cnt, sizeof(int), hipMemcpyDeviceToHost, st));
    if (he == hipSuccess) step(hipStreamSynchronize(st));
    cleanup();
    HIPCHK(he);
    if (n_accepted) *n_accepted = cnt;
    return SGA_OK;
}

}  // extern "C"
