// sga_state.cpp -- state access, checkpoint / resume, measurement and description entry points of the C ABI
// (include/sga.h): nothing here launches a sweep.
#include "sga_engine_impl.h"

extern "C" {

int sga_probe_read_bandwidth(int device, int64_t bytes, int reps, double *gb_per_s) {
    if (!gb_per_s || bytes < (1 << 20) || reps < 1) return fail(SGA_ERR_INVALID, "bad probe arguments");
    HIPCHK(hipSetDevice(device));
    bytes &= ~(int64_t)15;
    void *buf = nullptr;
    float *sink = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t he = hipMalloc(&buf, (size_t)bytes);
    if (he == hipSuccess) he = hipMalloc(&sink, sizeof(float));
    if (he == hipSuccess) he = hipMemset(buf, 0, (size_t)bytes);
    if (he == hipSuccess) he = hipEventCreate(&e0);
    if (he == hipSuccess) he = hipEventCreate(&e1);
    if (he == hipSuccess) he = sga::launch_probe_read(buf, bytes, sink, nullptr);  // warm-up
    if (he == hipSuccess) he = hipEventRecord(e0, nullptr);
    for (int i = 0; i < reps && he == hipSuccess; ++i) he = sga::launch_probe_read(buf, bytes, sink, nullptr);
    if (he == hipSuccess) he = hipEventRecord(e1, nullptr);
    if (he == hipSuccess) he = hipEventSynchronize(e1);
    float ms = 0.0f;
    if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    dev_free(buf);
    dev_free(sink);
    if (he != hipSuccess) return fail(SGA_ERR_DEVICE, hipGetErrorString(he));
    *gb_per_s = (double)bytes * reps / ((double)ms * 1e-3) / 1e9;
    return SGA_OK;
}

// ---- state access -------------------------------------------------------------------------
int sga_get_energies(sga_engine *e, double *out) {
    if (!e || !out) return fail(SGA_ERR_INVALID, "NULL argument");
    if (e->R <= 0) return fail(SGA_ERR_INVALID, "no replicas");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(out, e->energy, sizeof(double) * e->R, hipMemcpyDefault, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return SGA_OK;
}

int sga_get_temperatures(sga_engine *e, double *out) {
    if (!e || !out) return fail(SGA_ERR_INVALID, "NULL argument");
    if (e->R <= 0) return fail(SGA_ERR_INVALID, "no replicas");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(out, e->rep_temp, sizeof(double) * e->R, hipMemcpyDefault, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return SGA_OK;
}

int sga_get_spins(sga_engine *e, int r, int8_t *out) {
    if (!e || !out) return fail(SGA_ERR_INVALID, "NULL argument");
    if (e->R <= 0 || r >= e->R) return fail(SGA_ERR_INVALID, "bad replica index");
    HIPCHK(hipSetDevice(e->device));
    if (r >= 0) {
        HIPCHK(hipMemcpyAsync(out, e->spins + (long long)r * e->sstride, (size_t)spins_of(e, r),
                              hipMemcpyDefault, e->stream));
    } else {
        HIPCHK(hipMemcpy2DAsync(out, (size_t)e->n, e->spins, (size_t)e->sstride, (size_t)e->n,
                                (size_t)e->R, hipMemcpyDefault, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return SGA_OK;
}

int sga_set_spins(sga_engine *e, int r, const int8_t *s) {
    if (!e || !s) return fail(SGA_ERR_INVALID, "NULL argument");
    if (e->R <= 0 || r < 0 || r >= e->R) return fail(SGA_ERR_INVALID, "bad replica index");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemsetAsync(e->spins + (long long)r * e->sstride, 0, (size_t)e->sstride, e->stream));
    HIPCHK(hipMemcpyAsync(e->spins + (long long)r * e->sstride, s, (size_t)spins_of(e, r), hipMemcpyDefault,
                          e->stream));
    e->fields_valid = false;
    int rc = recompute_energy_range(e, r, 1);
    if (rc != SGA_OK) return rc;
    HIPCHK(sga::launch_copy_best(e->energy + r, e->spins + (long long)r * e->sstride,
                                 e->best_energy + r, e->best_spins + (long long)r * e->sstride,
                                 e->sstride, 1, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return SGA_OK;
}

int sga_get_best(sga_engine *e, int r, double *energy, int8_t *spins, int *r_out) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (e->R <= 0 || r >= e->R) return fail(SGA_ERR_INVALID, "bad replica index");
    HIPCHK(hipSetDevice(e->device));
    std::vector<double> be((size_t)e->R);
    HIPCHK(hipMemcpyAsync(be.data(), e->best_energy, sizeof(double) * e->R, hipMemcpyDeviceToHost,
                          e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (r < 0) {
        r = 0;
        for (int i = 1; i < e->R; ++i)
            if (be[i] < be[r]) r = i;
    }
    if (energy) *energy = be[r];
    if (r_out) *r_out = r;
    if (spins) {
        HIPCHK(hipMemcpyAsync(spins, e->best_spins + (long long)r * e->sstride, (size_t)spins_of(e, r),
                              hipMemcpyDefault, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return SGA_OK;
}

int sga_reset_best(sga_engine *e) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (e->R <= 0) return fail(SGA_ERR_INVALID, "no replicas");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(sga::launch_copy_best(e->energy, e->spins, e->best_energy, e->best_spins, e->sstride,
                                 e->R, e->stream));
    return SGA_OK;
}

int sga_get_stats(sga_engine *e, int64_t *accepted, int64_t *attempted) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (e->R <= 0) return fail(SGA_ERR_INVALID, "no replicas");
    HIPCHK(hipSetDevice(e->device));
    if (accepted) {
        HIPCHK(hipMemcpyAsync(accepted, e->n_acc, sizeof(int64_t) * e->R, hipMemcpyDefault,
                              e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    if (attempted) {
        if (is_device_ptr(attempted)) return fail(SGA_ERR_INVALID, "attempted must be a host buffer");
        for (int i = 0; i < e->R; ++i)  // (ragged batches: e->attempted counts n_max per sweep)
            attempted[i] = e->ragged ? e->attempted / e->n * spins_of(e, i) : e->attempted;
    }
    return SGA_OK;
}

int sga_get_slot_map(sga_engine *e, int32_t *slot_to_rep) {
    if (!e || !slot_to_rep) return fail(SGA_ERR_INVALID, "NULL argument");
    if (e->n_ladders <= 0) return fail(SGA_ERR_INVALID, "no ladder");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(slot_to_rep, e->slot_to_rep, sizeof(int32_t) * e->Rg, hipMemcpyDefault,
                          e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return SGA_OK;
}

int sga_get_exchange_stats(sga_engine *e, int64_t *attempts, int64_t *accepts) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (e->n_ladders <= 0) return fail(SGA_ERR_INVALID, "no ladder");
    HIPCHK(hipSetDevice(e->device));
    if (attempts)
        HIPCHK(hipMemcpyAsync(attempts, e->ex_attempts, sizeof(int64_t) * e->Rg, hipMemcpyDefault,
                              e->stream));
    if (accepts)
        HIPCHK(hipMemcpyAsync(accepts, e->ex_accepts, sizeof(int64_t) * e->Rg, hipMemcpyDefault,
                              e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return SGA_OK;
}

int sga_snapshot(sga_engine *e, double *energies, int64_t *accepted, int32_t *slot_to_rep) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (e->R <= 0) return fail(SGA_ERR_INVALID, "no replicas");
    if (slot_to_rep && e->n_ladders <= 0) return fail(SGA_ERR_INVALID, "no ladder");
    HIPCHK(hipSetDevice(e->device));
    if (energies)
        HIPCHK(hipMemcpyAsync(energies, e->energy, sizeof(double) * e->R, hipMemcpyDefault, e->stream));
    if (accepted)
        HIPCHK(hipMemcpyAsync(accepted, e->n_acc, sizeof(int64_t) * e->R, hipMemcpyDefault, e->stream));
    if (slot_to_rep)
        HIPCHK(hipMemcpyAsync(slot_to_rep, e->slot_to_rep, sizeof(int32_t) * e->Rg, hipMemcpyDefault, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return SGA_OK;
}

int sga_set_seed(sga_engine *e, uint64_t seed) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    e->seed = seed;
    return SGA_OK;
}

int sga_get_sweep_counter(sga_engine *e, uint32_t *sweeps_done, uint32_t *exchange_rounds) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (sweeps_done) *sweeps_done = e->sweeps_done;
    if (exchange_rounds) *exchange_rounds = e->rounds;
    return SGA_OK;
}

int sga_set_sweep_counter(sga_engine *e, uint32_t sweeps_done, uint32_t exchange_rounds) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    e->sweeps_done = sweeps_done;
    e->rounds = exchange_rounds;
    return SGA_OK;
}

// ---- checkpoint / resume -------------------------------------------------------------------
// The blob is independent of the launch geometry: spins travel unpadded ([R][n]), so a state
// exported after sga_autotune / sga_set_tuning imports into an engine laid out for any other
// waves-per-replica.  (The chain itself does not depend on the geometry either: integer problems
// sum exactly, real-valued ones in the canonical chunk order of sweep_dense_impl.h.)
namespace {
struct StateHeader {
    uint64_t magic;
    int32_t version, n, R, Rg, replica0, n_ladders;
    uint32_t sweeps_done, rounds;
    uint64_t seed;
    int64_t attempted;
};
constexpr uint64_t STATE_MAGIC = 0x5347415354415445ull;  // "SGASTATE"
constexpr int32_t STATE_VERSION = 2;
// The blob of an sga_set_csr_shared engine is the one-model CSR blob; the header's version word carries the number of
// field vectors in its upper half (n_models - 1: 0 for every other kind of problem, whose blobs are what they were), so
// that a state goes back only into an engine with as many models.
int32_t state_version_word(const sga_engine *e) {
    return STATE_VERSION | (int32_t)((e->csr && e->shared_j ? (uint32_t)(e->n_models - 1) & 0x7FFFu : 0u) << 16);
}

uint64_t state_bytes(const sga_engine *e) {
    const uint64_t R = (uint64_t)e->R, Rg = (uint64_t)e->Rg, sb = R * (uint64_t)e->n;
    uint64_t total = sizeof(StateHeader) + 2 * sb + 3 * R * sizeof(double) + R * sizeof(uint64_t);
    if (e->n_ladders > 0) total += Rg * (sizeof(int32_t) + 2 * sizeof(int64_t));
    return total;
}
}  // namespace

int sga_export_state(sga_engine *e, void *buf, uint64_t capacity, uint64_t *needed) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (e->R <= 0) return fail(SGA_ERR_INVALID, "no replicas");
    const uint64_t total = state_bytes(e);
    if (needed) *needed = total;
    if (!buf) return SGA_OK;
    if (capacity < total) return fail(SGA_ERR_INVALID, "state buffer too small");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    unsigned char *p = static_cast<unsigned char *>(buf);
    StateHeader h{STATE_MAGIC, state_version_word(e), e->n, e->R, e->Rg, e->replica0, e->n_ladders,
                  e->sweeps_done, e->rounds, e->seed, (int64_t)e->attempted};
    std::memcpy(p, &h, sizeof(h));
    p += sizeof(h);
    auto pull = [&](const void *dev, size_t bytes) -> hipError_t {
        hipError_t r = hipMemcpy(p, dev, bytes, hipMemcpyDeviceToHost);
        p += bytes;
        return r;
    };
    const size_t R = (size_t)e->R, Rg = (size_t)e->Rg, sb = R * (size_t)e->n;
    // spins leave the padded device layout through a staging slot
    HIPCHK(e->scratch[1].reserve(sb));
    int8_t *stage = static_cast<int8_t *>(e->scratch[1].ptr);
    for (const int8_t *src : {e->spins, e->best_spins}) {
        HIPCHK(sga::launch_unpad_spins(src, e->sstride, stage, e->n, e->R, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(pull(stage, sb));
    }
    HIPCHK(pull(e->energy, R * sizeof(double)));
    HIPCHK(pull(e->best_energy, R * sizeof(double)));
    HIPCHK(pull(e->rep_temp, R * sizeof(double)));
    HIPCHK(pull(e->n_acc, R * sizeof(uint64_t)));
    if (e->n_ladders > 0) {
        HIPCHK(pull(e->slot_to_rep, Rg * sizeof(int32_t)));
        HIPCHK(pull(e->ex_attempts, Rg * sizeof(int64_t)));
        HIPCHK(pull(e->ex_accepts, Rg * sizeof(int64_t)));
    }
    return SGA_OK;
}

int sga_import_state(sga_engine *e, const void *buf, uint64_t size) {
    if (!e || !buf) return fail(SGA_ERR_INVALID, "NULL argument");
    if (e->R <= 0) return fail(SGA_ERR_INVALID, "initialise the replicas before importing a state");
    if (size < sizeof(StateHeader)) return fail(SGA_ERR_INVALID, "state blob truncated");
    StateHeader h;
    std::memcpy(&h, buf, sizeof(h));
    if (h.magic != STATE_MAGIC) return fail(SGA_ERR_INVALID, "not an engine state blob");
    if ((h.version & 0xFFFF) != STATE_VERSION) return fail(SGA_ERR_INVALID, "state blob of another engine version");
    if (h.version != state_version_word(e))
        return fail(SGA_ERR_INVALID, "state blob does not match this engine's problem (shared-coupling CSR batches: another "
                                     "number of models)");
    if (h.n != e->n || h.R != e->R || h.Rg != e->Rg || h.replica0 != e->replica0 ||
        h.n_ladders != e->n_ladders)
        return fail(SGA_ERR_INVALID, "state blob does not match this engine's problem / replicas / ladder");
    if (size != state_bytes(e)) return fail(SGA_ERR_INVALID, "state blob has the wrong size");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const unsigned char *p = static_cast<const unsigned char *>(buf) + sizeof(h);
    auto push = [&](void *dev, size_t bytes) -> hipError_t {
        hipError_t r = hipMemcpy(dev, p, bytes, hipMemcpyHostToDevice);
        p += bytes;
        return r;
    };
    const size_t R = (size_t)e->R, Rg = (size_t)e->Rg, sb = R * (size_t)e->n;
    HIPCHK(e->scratch[1].reserve(sb));
    int8_t *stage = static_cast<int8_t *>(e->scratch[1].ptr);
    for (int8_t *dst : {e->spins, e->best_spins}) {
        HIPCHK(push(stage, sb));
        HIPCHK(sga::launch_pad_spins(stage, e->n, dst, e->sstride, e->R, e->stream));
        if (e->ragged)  // (past a replica's model: padding, whatever the blob holds)
            HIPCHK(sga::launch_mask_spins_ragged(dst, e->sstride, e->R, (uint32_t)e->replica0, e->d_models,
                                                 e->Rg / e->n_models, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    HIPCHK(push(e->energy, R * sizeof(double)));
    HIPCHK(push(e->best_energy, R * sizeof(double)));
    HIPCHK(push(e->rep_temp, R * sizeof(double)));
    HIPCHK(push(e->n_acc, R * sizeof(uint64_t)));
    if (e->n_ladders > 0) {
        HIPCHK(push(e->slot_to_rep, Rg * sizeof(int32_t)));
        HIPCHK(push(e->ex_attempts, Rg * sizeof(int64_t)));
        HIPCHK(push(e->ex_accepts, Rg * sizeof(int64_t)));
    }
    e->sweeps_done = h.sweeps_done;
    e->rounds = h.rounds;
    e->seed = h.seed;
    e->attempted = h.attempted;
    e->fields_valid = false;
    return SGA_OK;
}

// ---- measurement --------------------------------------------------------------------------
int sga_enable_timing(sga_engine *e, int on) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    e->timing = on != 0;
    return SGA_OK;
}

int sga_get_kernel_time(sga_engine *e, int64_t *n_launches, double *total_ms, int reset) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (auto &p : e->events) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) {
            e->total_ms += ms;
            e->launches += 1;
        }
        (void)hipEventDestroy(p.first);
        (void)hipEventDestroy(p.second);
    }
    e->events.clear();
    if (n_launches) *n_launches = e->launches;
    if (total_ms) *total_ms = e->total_ms;
    if (reset) {
        e->launches = 0;
        e->total_ms = 0.0;
    }
    return SGA_OK;
}

int sga_describe(sga_engine *e, char *buf, int buflen) {
    if (!e || !buf || buflen <= 0) return fail(SGA_ERR_INVALID, "bad arguments");
    char tmp[640];
    char rest[96] = "";  // sga_set_groups_csr: the stored remainder
    if (e->groups && e->group_args.rest.nnz > 0)
        std::snprintf(rest, sizeof(rest), " rest_nnz=%lld rest_max_row=%d", e->group_args.rest.nnz, e->group_args.rest.max_row);
    if (e->groups)
        std::snprintf(tmp, sizeof(tmp),
                      "groups n=%d n_groups=%d largest_group=%d memberships=%lld max_memberships=%d%s R=%d waves_per_replica=%d "
                      "sstride=%d path=groups couplings=implicit (group sums as %s in LDS, 0 coupling bytes per proposal%s) "
                      "acc=f32-exact grid=2^%d lds_bytes=%zu",
                      e->n, e->group_args.n_groups, e->g_max_size, e->g_memberships, e->g_kmax, rest, e->R, e->waves, e->sstride,
                      e->group_args.wide ? "int32" : "int16",
                      e->group_args.rest.nnz > 0 ? " for the groups; stored remainder rows walked once per candidate and window" : "",
                      -e->g_exp,
                      sga::groups_lds_bytes(e->sstride > 0 ? e->sstride : (e->n + 127) / 128 * 128, e->group_args.n_groups,
                                            e->group_args.wide));
    else if (e->tsp)
        std::snprintf(tmp, sizeof(tmp),
                      "tsp n_cities=%d n=%d R=%d waves_per_replica=%d passes=%d couplings=implicit "
                      "(2 x %d-byte distance rows per update) acc=%s lds_bytes=%zu",
                      e->tsp_args.n_cities, e->n, e->R, e->tsp_waves, e->tsp_passes, 4 * e->tsp_args.n_cities,
                      !e->tsp_args.f64 ? "f32-exact" : (e->tsp_exact ? "f64-exact" : "f64"),
                      sga::tsp_lds_bytes(e->tsp_args.n_cities, e->tsp_args.npad));
    else if (e->ragged)
        std::snprintf(tmp, sizeof(tmp),
                      "csr batch models=%d n=%d..%d nnz=%lld R=%d waves_per_replica=1 replicas_per_block=%d sstride=%d "
                      "path=%s table_m=%d spins=lds-int8 form=narrow-ragged%s",
                      e->n_models, *std::min_element(e->model_n.begin(), e->model_n.end()), e->n, e->nnz, e->R,
                      sga::csr_waves_per_block(e->sstride, e->table_m), e->sstride,
                      (e->csr_acc == sga::CSR_ACC_F32_TABLE && e->table_m > 0) ? (e->table_scale == 2 ? "half-integer-fast" : "integer-fast")
                      : e->csr_acc <= sga::CSR_ACC_F32 ? "general acc=f32-exact"
                      : e->csr_acc == sga::CSR_ACC_F64 ? "general acc=f64-exact"
                                                       : "general acc=f64-canonical",
                      e->table_m,
                      // (option "ragged_field_cache" with the cache requested: the sweep form is named below)
                      (e->opt[OPT_RAGGED_FIELD_CACHE] == 1 && e->field_cache != SGA_FIELD_CACHE_OFF)
                          ? "" : " sweep=streaming(no field cache for ragged batches)");
    else if (e->csr)
        std::snprintf(tmp, sizeof(tmp),
                      "csr n=%d %snnz=%lld R=%d waves_per_replica=%d replicas_per_block=%d sstride=%d "
                      "path=%s table_m=%d spins=%s",
                      e->n, e->shared_j ? ("shared-J models=" + std::to_string(e->n_models) + " ").c_str() : "", e->nnz, e->R, e->waves,
                      e->big_form == 2 ? sga::csr_bits_waves_per_block(e->sstride, e->table_m)
                                       : ((e->waves > 1 || e->big) ? 1 : sga::csr_waves_per_block(e->sstride, e->table_m)),
                      e->sstride,
                      (e->csr_acc == sga::CSR_ACC_F32_TABLE && e->table_m > 0) ? (e->table_scale == 2 ? "half-integer-fast" : "integer-fast")
                      : e->csr_acc == sga::CSR_ACC_F32_TABLE ? "general acc=f32-exact"
                      : e->csr_acc == sga::CSR_ACC_F32     ? "general acc=f32-exact"
                      : e->csr_acc == sga::CSR_ACC_F64     ? "general acc=f64-exact"
                                                           : "general acc=f64-canonical",
                      e->table_m,
                      e->big ? "lds-bits" : "lds-int8");
    else
        std::snprintf(tmp, sizeof(tmp),
                      "dense n=%d %smodels=%d storage=%s acc=%s R=%d waves_per_replica=%d "
                      "chunks_per_wave=%d%s ld=%lld row_bytes=%lld table_m=%d look_ahead=%d",
                      e->n, e->shared_j ? "shared-J " : "", e->n_models, e->use_t2 ? "t2" : (e->want_i8 ? "i8" : "f32"),
                      e->want_i8 ? "i32" : (e->acc64 ? (e->acc_canon ? "f64-canonical" : "f64-exact") : "f32"), e->R,
                      e->use_t2 ? e->waves_t2 : e->waves, e->use_t2 ? e->cpw_t2 : e->cpw,
                      (e->use_t2 ? e->cpw_t2 > sga::T2_MAX_CPW : e->cpw > sga::MAX_CPW) ? "(streaming)" : "", e->ld,
                      e->use_t2 ? t2_row_bits(e->n) / 4 : e->ldj * (e->want_i8 ? 1 : 4), e->table_m,
                      (e->table_m > 0 && e->opt[OPT_LOOK_AHEAD] != 0)
                          ? sga::dense_look_ahead(e->use_t2, e->want_i8, e->acc64,
                                                  e->use_t2 ? e->cpw_t2 : e->cpw,
                                                  e->use_t2 ? e->waves_t2 : e->waves, e->R)
                          : 1);
    if (!e->csr && !e->implicit() && e->field_cache == SGA_FIELD_CACHE_OFF) {  // production sweeps in row-shared windows
        const int rw = row_shared_window(e, true);
        if (rw > 0) {
            int grid = 0;
            const int pl = row_shared_form_planes(e, &grid);
            // (Metropolis lines name no rule; Glauber and heat bath decide with the general rule: " rule=...")
            const char *rule = e->rule == SGA_RULE_GLAUBER ? " rule=glauber" : e->rule == SGA_RULE_HEAT_BATH ? " rule=heat-bath" : "";
            if (grid)  // option "row_shared_grid": J on the grid 2^-k, the planes are those of 2^k J
                std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp), " sweep=row-shared(W=%d planes=%d grid=2^-%d%s)", rw,
                              pl, grid - 1, rule);
            else
                std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp), " sweep=row-shared(W=%d planes=%d%s)", rw, pl, rule);
            if (sga::row_shared_resident(e->want_i8, pl))  // (the bytes the form's first sweep adds, once per problem)
                std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp), " rs_fields=resident-planes(%zuB)",
                              sga::row_shared_plane_bytes(e->n, pl));
            else
                std::strncat(tmp, " rs_fields=on-chip-conversion", sizeof(tmp) - std::strlen(tmp) - 1);
            if (e->win.jp) {  // (the planes exist: whether the rows are sign-only is known) option "row_shared_fields"
                const char *why = nullptr;
                const sga::RowSharedTiles t = row_shared_tiles(e, &why);
                if (t.S > 0)
                    std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp), " rs_tiles=%d-sites%s", t.S,
                                  t.ones ? "(sign-only)" : "");
                else
                    std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp), " rs_tiles=no(%s)", why ? why : "-");
            }
        }
    }
    if (const sga::SeqWindows sq = sequential_windows(e); sq.W > 0)  // sga_set_sequential_windows: SGA_SITE_SEQUENTIAL sweeps
        std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp), " sweep=seq-windows(W=%d)", sq.W);
    if (e->csr && !e->ragged && csr_updates_per_step(e) >= 4 && e->waves <= 1 && (e->big_form == 0 || e->big_form == 2) && e->rowptr)
        std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp), " updates_per_step=%d", csr_updates_per_step(e));
    if (e->csr && e->from_dense) std::strncat(tmp, " source=dense-matrix(sparse)", sizeof(tmp) - std::strlen(tmp) - 1);
    if (e->csr && e->slotted)
        std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp),
                      " rows=64-entry-slots(+%.1f%%) longest_row_slots=%lld",
                      e->nnz > 0 ? 100.0 * (double)(e->layout_entries - e->nnz) / (double)e->nnz : 0.0,
                      (e->max_row_len + 63) / 64);
    if (e->csr && e->big_form == 1 && e->cvp && e->csr_storage_latched != SGA_CSR_STORAGE_F32)
        std::strncat(tmp, " entries=packed-32bit", sizeof(tmp) - std::strlen(tmp) - 1);
    if (!e->consistent_dE) std::strncat(tmp, " energy=recomputed-per-sweep", sizeof(tmp) - std::strlen(tmp) - 1);
    if (e->ragged) {
        // option "ragged_field_cache": the int16 cached-field form over the batch, or why it streams
        if (e->opt[OPT_RAGGED_FIELD_CACHE] == 1 && e->field_cache != SGA_FIELD_CACHE_OFF) {
            if (!clf_active(e))
                std::strncat(tmp, " sweep=streaming(the batch does not qualify for cached local fields)", sizeof(tmp) - std::strlen(tmp) - 1);
            else if (e->field_cache == SGA_FIELD_CACHE_ON && e->clf_fx_bits)
                std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp),
                              " sweep=cached-local-fields(ragged models=%d: int%d fixed-point dynamic fields, k=%d, of each replica's "
                              "model in LDS, %d waves per replica, row entries read on accept only)",
                              e->n_models, e->clf_fx_bits, e->clf_fx_k, sga_route::clf_csr_waves(route_query_of(e)));
            else if (e->clf_fx_bits)
                std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp),
                              " sweep=auto(ragged cached local fields models=%d, int%d fixed-point, k=%d, while the hottest replica "
                              "accepts little; now: %s)",
                              e->n_models, e->clf_fx_bits, e->clf_fx_k,
                              (!e->routing.unavailable && e->routing.n_cached > 0) ? "cached" : "one row per proposal");
            else if (e->field_cache == SGA_FIELD_CACHE_ON)
                std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp),
                              " sweep=cached-local-fields(ragged: int16 dynamic fields of each replica's model in LDS, %d waves per "
                              "replica, scale=%d, row entries read on accept only)",
                              sga_route::clf_csr_waves(route_query_of(e)), e->table_scale);
            else
                std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp),
                              " sweep=auto(ragged cached local fields while the hottest replica accepts little; now: %s)",
                              (!e->routing.unavailable && e->routing.n_cached > 0) ? "cached" : "one row per proposal");
        }
    } else if (clf_active(e) && e->csr) {
        if (e->field_cache == SGA_FIELD_CACHE_ON && e->clf_fx_bits)
            std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp),
                          " sweep=cached-local-fields(int%d fixed-point dynamic fields, k=%d, in LDS, row entries read on accept only)",
                          e->clf_fx_bits, e->clf_fx_k);
        else if (e->field_cache == SGA_FIELD_CACHE_ON)
            std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp),
                          " sweep=cached-local-fields(int16 dynamic fields in LDS, row entries read on accept only)");
        else if (e->clf_fx_bits)
            std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp),
                          " sweep=auto(cached local fields, int%d fixed-point, k=%d, while the hottest replica accepts little; now: %s)",
                          e->clf_fx_bits, e->clf_fx_k, (!e->routing.unavailable && e->routing.n_cached > 0) ? "cached" : "one row per proposal");
        else
            std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp),
                          " sweep=auto(cached local fields while the hottest replica accepts little; now: %s)",
                          (!e->routing.unavailable && e->routing.n_cached > 0) ? "cached" : "one row per proposal");
    } else if (clf_active(e) && e->clf_fx_bits) {  // dense couplings, option "clf_fixed_point"
        if (e->field_cache == SGA_FIELD_CACHE_ON)
            std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp),
                          " sweep=cached-local-fields(int%d fixed-point, k=%d, in LDS, %d wave(s) per replica, row read on accept only)",
                          e->clf_fx_bits, e->clf_fx_k, sga::sweep_clf_waves(e->ldj, e->want_i8, e->R, e->cus, (int)e->opt[OPT_CLF_WAVES]));
        else
            std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp),
                          " sweep=auto(cached local fields, int%d fixed-point, k=%d, per replica by its own acceptance; now: %d of "
                          "%d replica(s) cached, the rest one row per proposal)",
                          e->clf_fx_bits, e->clf_fx_k, e->routing.unavailable ? 0 : e->routing.n_cached, e->R);
        if (e->n_models > 1)  // option "batch_fixed_point": the batch, its width and its one k
            std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp), " cached-batch(models=%d fields=int%d k=%d)",
                          e->n_models, e->clf_fx_bits, e->clf_fx_k);
    } else if (clf_active(e)) {
        if (e->field_cache == SGA_FIELD_CACHE_ON)
            std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp),
                          " sweep=cached-local-fields(int%d in LDS, %d wave(s) per replica%s, row read on accept only)",
                          e->clf_bits, sga::sweep_clf_waves(e->ldj, e->want_i8, e->R, e->cus, (int)e->opt[OPT_CLF_WAVES]),
                          e->routing.wide ? " -- now 8: the launch is its hottest replica's chain" : "");
        else
            std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp),
                          " sweep=auto(cached local fields, int%d in LDS, per replica by its own acceptance; now: %d of %d "
                          "replica(s) cached%s, the rest one row per proposal)",
                          e->clf_bits, e->routing.unavailable ? 0 : e->routing.n_cached, e->R,
                          (!e->routing.unavailable && e->routing.wide) ? " at 8 waves each" : "");
        if (e->n_models > 1)  // many-model batches: which form ran is visible (batch-wide scale and field width)
            std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp), " cached-batch(models=%d scale=%d)", e->n_models,
                          e->clf_scale);
    }
    // Replica groups of the row-shared sweep (sga_set_replica_groups), behind everything else: the count where more than one
    // runs; where the caller asked for more and the form admits none, why.  One group by the rule: the line as it was.
    if (e->R > 0) {
        int rw = 0;
        sga::RowSharedTiles t{};
        if (!e->csr && !e->implicit() && e->field_cache == SGA_FIELD_CACHE_OFF && (rw = row_shared_window(e, true)) > 0 && e->win.jp) {
            t = row_shared_tiles(e, nullptr);
            if (t.S > 0 && sga::row_shared_tile_plan(e->n, rw, t.S, e->R).rg == 0) t = sga::RowSharedTiles{};  // (as plan_windows)
        }
        const char *why = nullptr;
        const int G = replica_groups(e, rw, t, false, &why);
        if (G > 1) std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp), " groups=%d", G);
        else if (why && e->win.groups > 1) std::snprintf(tmp + std::strlen(tmp), sizeof(tmp) - std::strlen(tmp), " groups=no(%s)", why);
    }
    std::snprintf(buf, (size_t)buflen, "%s", tmp);
    return SGA_OK;
}

int sga_problem_checksum(sga_engine *e, uint64_t *out) {
    if (!e || !out) return fail(SGA_ERR_INVALID, "NULL argument");
    if (e->n <= 0) return fail(SGA_ERR_INVALID, "no couplings set");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(e->point_out.reserve(2 * sizeof(unsigned long long)));
    unsigned long long *d = static_cast<unsigned long long *>(e->point_out.ptr);
    HIPCHK(hipMemsetAsync(d, 0, 2 * sizeof(unsigned long long), e->stream));
    // what the sweep kernels read: the packed matrix | the entry layout | the distance tables; then h
    if (e->groups) {  // extents, members, coefficients (h below)
        const int G = e->group_args.n_groups;
        HIPCHK(sga::launch_checksum(e->g_member_ptr, 8ll * (G + 1), d, e->stream));
        if (e->g_memberships > 0) HIPCHK(sga::launch_checksum(e->g_members, 4ll * e->g_memberships, d, e->stream));
        if (G > 0) HIPCHK(sga::launch_checksum(e->g_coeff, 4ll * G, d, e->stream));
        if (e->group_args.rest.nnz > 0) {  // the stored remainder: extents, then (column, value) entries
            HIPCHK(sga::launch_checksum(e->g_rptr, 4ll * (e->n + 1), d, e->stream));
            HIPCHK(sga::launch_checksum(e->g_rent, 8ll * e->group_args.rest.nnz, d, e->stream));
        }
    } else if (e->tsp) {
        const long long bytes = 4ll * e->tsp_args.n_cities * e->tsp_args.npad;
        HIPCHK(sga::launch_checksum(e->nd4, bytes, d, e->stream));
        HIPCHK(sga::launch_checksum(e->nd4t, bytes, d, e->stream));
    } else if (e->csr) {
        HIPCHK(sga::launch_checksum(e->cv, 8ll * e->layout_entries, d, e->stream));
        const long long rows = e->ragged ? e->n_rows : e->n;
        HIPCHK(sga::launch_checksum(e->rowptr64, 8ll * (rows + 1), d, e->stream));
        if (e->ragged) HIPCHK(sga::launch_checksum(e->d_models, 8ll * e->n_models, d, e->stream));  // the models' sizes
    } else {
        // (sga_set_dense_shared: the one matrix once, every model's h below)
        HIPCHK(sga::launch_checksum(e->J_packed, (long long)(e->shared_j ? 1 : e->n_models) * e->n * e->ldj * (e->want_i8 ? 1 : 4), d,
                                    e->stream));
    }
    HIPCHK(sga::launch_checksum(e->h, e->ragged ? 4ll * e->n_rows : 4ll * e->n * (e->implicit() ? 1 : e->n_models), d + 1, e->stream));
    unsigned long long host[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(host, d, sizeof(host), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    *out = host[0] ^ ((host[1] << 17) | (host[1] >> 47)) ^ ((uint64_t)(uint32_t)e->n << 32);
    // (sga_set_csr_shared: the layout once, all of H above, and the number of models)
    if (e->csr && e->shared_j) *out ^= (uint64_t)(uint32_t)e->n_models * 0x9E3779B97F4A7C15ull;
    return SGA_OK;
}

int sga_get_geometry(sga_engine *e, int *waves_per_replica, int *chunks_per_wave) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (waves_per_replica) *waves_per_replica = (!e->csr && !e->implicit() && e->use_t2) ? e->waves_t2 : e->waves;
    if (chunks_per_wave) *chunks_per_wave = (!e->csr && !e->implicit() && e->use_t2) ? e->cpw_t2 : e->cpw;
    return SGA_OK;
}

int sga_get_energies_async(sga_engine *e, double *out_device) {
    if (!e || !out_device) return fail(SGA_ERR_INVALID, "NULL argument");
    if (e->R <= 0) return fail(SGA_ERR_INVALID, "no replicas");
    if (!is_device_ptr(out_device)) return fail(SGA_ERR_INVALID, "sga_get_energies_async needs a device buffer");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(out_device, e->energy, sizeof(double) * e->R, hipMemcpyDeviceToDevice, e->stream));
    return SGA_OK;
}

// ---- replica observables (observables.hip) --------------------------------------------------
// Read only, and no state of their own: the result of a host `out` goes through the point_out slot, a host `cfg`
// through point_sites (both grow-only, so the steady-state call allocates nothing), and nothing else of the engine is
// written -- not the spins, fields, counters, bests, window plan or last_kernel.
namespace {
const int8_t *observed_rows(const sga_engine *e, int which) { return which == SGA_SPINS_BEST ? e->best_spins : e->spins; }
bool observed_which(int which) { return which == SGA_SPINS_CURRENT || which == SGA_SPINS_BEST; }
const char *observables_ready(const sga_engine *e) {
    if (e->n <= 0) return "no couplings set";
    if (e->R <= 0 || !e->spins || !e->best_spins) return "no replicas";
    return nullptr;
}

// out[a * ldq + b] = sum_{i < n} A_a[i] B_b[i], A the local replicas' rows; B on the device.  Every argument is checked
// by the caller; the work goes on the engine's stream, and a host `out` is waited for.
int observables_product(sga_engine *e, const int8_t *A, const int8_t *B, long long ldb, int rows_b, bool symmetric,
                        int32_t *out, int64_t ldq) {
    sga::ObservablesArgs a{};
    a.A = A, a.B = B;
    a.lda = e->sstride, a.ldb = ldb;
    a.rows_a = e->R, a.rows_b = rows_b, a.n = e->n;
    a.symmetric = symmetric ? 1 : 0;
    a.plan = sga::observables_plan(e->n, e->R, rows_b, e->cus);
    const bool on_device = is_device_ptr(out);
    if (on_device) {
        a.out = out, a.ldq = ldq;
    } else {
        HIPCHK(e->point_out.reserve((size_t)e->R * (size_t)rows_b * sizeof(int32_t)));
        a.out = static_cast<int *>(e->point_out.ptr), a.ldq = rows_b;
    }
    if (a.plan.ksplit > 1)  // the K ranges add into the result
        HIPCHK(hipMemset2DAsync(a.out, (size_t)a.ldq * sizeof(int32_t), 0, (size_t)rows_b * sizeof(int32_t), (size_t)e->R, e->stream));
    HIPCHK(sga::launch_observables_product(a, e->stream));
    if (!on_device) {
        HIPCHK(hipMemcpy2DAsync(out, (size_t)ldq * sizeof(int32_t), a.out, (size_t)rows_b * sizeof(int32_t),
                                (size_t)rows_b * sizeof(int32_t), (size_t)e->R, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return SGA_OK;
}
}  // namespace

int sga_get_magnetizations(sga_engine *e, int which, int32_t *out) {
    if (!e || !out) return fail(SGA_ERR_INVALID, "NULL argument");
    if (const char *why = observables_ready(e)) return fail(SGA_ERR_INVALID, why);
    if (!observed_which(which)) return fail(SGA_ERR_INVALID, "which must be SGA_SPINS_CURRENT or SGA_SPINS_BEST");
    HIPCHK(hipSetDevice(e->device));
    const bool on_device = is_device_ptr(out);
    int *d = out;
    if (!on_device) {
        HIPCHK(e->point_out.reserve((size_t)e->R * sizeof(int32_t)));
        d = static_cast<int *>(e->point_out.ptr);
    }
    HIPCHK(sga::launch_observables_row_sums(observed_rows(e, which), e->sstride, e->n, e->R, d, e->stream));
    if (!on_device) {
        HIPCHK(hipMemcpyAsync(out, d, (size_t)e->R * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return SGA_OK;
}

int sga_get_overlaps(sga_engine *e, int which_a, int which_b, int32_t *out, int64_t ldq) {
    if (!e || !out) return fail(SGA_ERR_INVALID, "NULL argument");
    if (const char *why = observables_ready(e)) return fail(SGA_ERR_INVALID, why);
    if (!observed_which(which_a) || !observed_which(which_b))
        return fail(SGA_ERR_INVALID, "which_a / which_b must be SGA_SPINS_CURRENT or SGA_SPINS_BEST");
    if (ldq < e->R) return fail(SGA_ERR_INVALID, "ldq is smaller than the number of local replicas");
    HIPCHK(hipSetDevice(e->device));
    return observables_product(e, observed_rows(e, which_a), observed_rows(e, which_b), e->sstride, e->R, which_a == which_b, out, ldq);
}

int sga_get_overlaps_with(sga_engine *e, int which, const int8_t *cfg, int64_t ld, int count, int32_t *out, int64_t ldq) {
    if (!e || !out) return fail(SGA_ERR_INVALID, "NULL argument");
    if (const char *why = observables_ready(e)) return fail(SGA_ERR_INVALID, why);
    if (!observed_which(which)) return fail(SGA_ERR_INVALID, "which must be SGA_SPINS_CURRENT or SGA_SPINS_BEST");
    if (count < 0) return fail(SGA_ERR_INVALID, "count is negative");
    if (count > 0 && !cfg) return fail(SGA_ERR_INVALID, "cfg is NULL");
    if (ld < e->n) return fail(SGA_ERR_INVALID, "ld is smaller than n");
    if (ldq < count) return fail(SGA_ERR_INVALID, "ldq is smaller than count");
    if (count == 0) return SGA_OK;
    HIPCHK(hipSetDevice(e->device));
    const int8_t *B = cfg;
    long long ldb = ld;
    if (!is_device_ptr(cfg)) {  // staged with rows 16 bytes apart: the product's wide loads (the pad is masked, not read as data)
        ldb = ((long long)e->n + 15) / 16 * 16;
        HIPCHK(e->point_sites.reserve((size_t)count * (size_t)ldb));
        HIPCHK(hipMemcpy2DAsync(e->point_sites.ptr, (size_t)ldb, cfg, (size_t)ld, (size_t)e->n, (size_t)count, hipMemcpyHostToDevice,
                                e->stream));
        B = static_cast<const int8_t *>(e->point_sites.ptr);
    }
    return observables_product(e, observed_rows(e, which), B, ldb, count, false, out, ldq);
}

// ---- isoenergetic cluster moves (cluster_moves.hip) ------------------------------------------
// No state of their own: a host pair list is staged in scratch slot 7 (as sga_exchange_pairs stages its list), the
// energies before the move and the touched flags lie in slot 6, a host `sizes` goes through point_out.
namespace {
// nullptr where the engine's problem is one the move serves, else why not; *code: the error to return
const char *cluster_refusal(const sga_engine *e, int *code) {
    *code = SGA_ERR_INVALID;
    if (e->n <= 0) return "no couplings set";
    if (e->R <= 0 || !e->spins) return "no replicas";
    *code = SGA_ERR_UNSUPPORTED;
    if (e->tsp) return "cluster moves are not implemented for sga_set_tsp problems (no stored rows to walk)";
    if (e->groups) return "cluster moves are not implemented for sga_set_groups / sga_set_groups_csr problems (no stored rows to walk)";
    if (e->ragged) return "cluster moves are not implemented for ragged CSR batches";
    if (!e->csr || !e->rowptr64 || !e->cv)
        return "cluster moves need sparse (CSR) couplings: on dense couplings the component is always every differing site";
    if (e->n > sga::CLUSTER_MAX_N) return "cluster moves: the bitmaps of n sites do not fit LDS (n / 2 bytes of 160 KiB)";
    return nullptr;
}

// The move over `count` pairs (a.pairs or a.slot_to_rep set by the caller), the energies and the bests behind it.
int cluster_move_run(sga_engine *e, sga::ClusterArgs a, int count, uint32_t round, int32_t *sizes) {
    hipStream_t st = e->stream;
    const size_t R = (size_t)e->R;
    HIPCHK(e->scratch[6].reserve(R * (sizeof(double) + sizeof(int))));
    double *saved = static_cast<double *>(e->scratch[6].ptr);
    int *touched = reinterpret_cast<int *>(saved + R);
    const bool sizes_on_device = sizes && is_device_ptr(sizes);
    if (sizes && !sizes_on_device) HIPCHK(e->point_out.reserve((size_t)count * sizeof(int32_t)));
    HIPCHK(hipMemcpyAsync(saved, e->energy, R * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemsetAsync(touched, 0, R * sizeof(int), st));
    a.spins = e->spins;
    a.rowptr64 = e->rowptr64;
    a.cv = e->cv;
    a.n_accepted = e->n_acc;
    a.sizes = !sizes ? nullptr : sizes_on_device ? sizes : static_cast<int *>(e->point_out.ptr);
    a.touched = touched;
    a.n = e->n;
    a.sstride = e->sstride;
    a.R = e->R;
    a.count = count;
    a.replica0 = (uint32_t)e->replica0;
    a.seed_lo = (uint32_t)e->seed;
    a.seed_hi = (uint32_t)(e->seed >> 32);
    a.round = round;
    HIPCHK(sga::launch_cluster_moves(a, st));
    e->fields_valid = false;
    // the whole range, as sga_recompute_energies forms it: the same pass, so the same bits; the replicas whose spins did
    // not change get their energies back
    int rc = recompute_energy_range(e, 0, e->R);
    if (rc != SGA_OK) return rc;
    HIPCHK(sga::launch_cluster_finish(touched, saved, e->energy, e->spins, e->best_energy, e->best_spins, e->sstride, e->R, st));
    if (sizes && !sizes_on_device) {
        HIPCHK(hipMemcpyAsync(sizes, a.sizes, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return SGA_OK;
}
}  // namespace

int sga_cluster_move_pairs(sga_engine *e, const int32_t *pairs, int count, uint32_t round, int32_t *sizes) {
    if (!e || !pairs) return fail(SGA_ERR_INVALID, "NULL argument");
    int code = SGA_OK;
    if (const char *why = cluster_refusal(e, &code)) return fail(code, why);
    if (count < 0) return fail(SGA_ERR_INVALID, "count is negative");
    if (is_device_ptr(pairs)) return fail(SGA_ERR_INVALID, "pairs must be a host buffer");
    std::vector<unsigned char> seen((size_t)e->R);
    const int reps_per_model = e->shared_j && e->n_models > 1 ? e->Rg / e->n_models : 0;
    if (const char *why = sga::cluster_pairs_check(pairs, count, e->R, e->replica0, reps_per_model, seen.data()))
        return fail(SGA_ERR_INVALID, why);
    if (count == 0) return SGA_OK;
    HIPCHK(hipSetDevice(e->device));
    // (a pageable host list: the copy has left the caller's buffer when the call returns)
    HIPCHK(e->scratch[7].reserve((size_t)2 * count * sizeof(int32_t)));
    HIPCHK(hipMemcpyAsync(e->scratch[7].ptr, pairs, (size_t)2 * count * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    sga::ClusterArgs a{};
    a.pairs = static_cast<const int32_t *>(e->scratch[7].ptr);
    return cluster_move_run(e, a, count, round, sizes);
}

int sga_cluster_move_ladders(sga_engine *e, int slot_lo, int slot_hi, uint32_t round, int32_t *sizes) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    int code = SGA_OK;
    if (const char *why = cluster_refusal(e, &code)) return fail(code, why);
    if (e->n_ladders <= 0 || !e->slot_to_rep) return fail(SGA_ERR_INVALID, "no ladder (call sga_set_ladder)");
    if (e->n_ladders % 2 != 0) return fail(SGA_ERR_INVALID, "cluster moves between ladders need an even number of ladders");
    if (e->R != e->Rg) return fail(SGA_ERR_INVALID, "cluster moves between ladders need every replica on this rank (R_local == R_global)");
    const int L = e->Rg / e->n_ladders;
    if (slot_lo < 0 || slot_hi > L || slot_lo > slot_hi) return fail(SGA_ERR_INVALID, "slot range outside [0, slots)");
    if (e->shared_j && e->n_models > 1) {  // a ladder's slots hold its own L replicas: both ladders under one field vector
        const int reps = e->Rg / e->n_models;
        for (int c = 0; c < e->n_ladders / 2; ++c)
            if ((2 * c * L) / reps != ((2 * c + 2) * L - 1) / reps)
                return fail(SGA_ERR_INVALID, "shared-coupling CSR batch: ladders " + std::to_string(2 * c) + " and " +
                                                 std::to_string(2 * c + 1) + " lie under two models (their field vectors differ)");
    }
    if (slot_lo == slot_hi) return SGA_OK;
    HIPCHK(hipSetDevice(e->device));
    sga::ClusterArgs a{};
    a.slot_to_rep = e->slot_to_rep;
    a.L = L;
    a.slot_lo = slot_lo;
    a.n_slots = slot_hi - slot_lo;
    return cluster_move_run(e, a, (e->n_ladders / 2) * a.n_slots, round, sizes);
}

// ---- population annealing: the resampling step (resample.hip) ---------------------------------
// No state of its own: the plan's arrays (sga_kernels.h, resample_scratch) lie in scratch slot 6 with the staged dbeta
// behind them, the outputs leave from there; the two kernels follow each other on the engine's stream.
int sga_resample(sga_engine *e, int n_populations, const double *dbeta, uint32_t round, int32_t *parents, double *shift,
                 uint64_t *weight_sum) {
    if (!e || !dbeta) return fail(SGA_ERR_INVALID, "NULL argument");
    if (e->n <= 0) return fail(SGA_ERR_INVALID, "no couplings set");
    if (e->R <= 0 || !e->spins || !e->best_spins) return fail(SGA_ERR_INVALID, "no replicas");
    if (is_device_ptr(dbeta)) return fail(SGA_ERR_INVALID, "dbeta must be a host buffer");
    if (const char *why = sga::resample_check(n_populations, dbeta, e->R, e->Rg, e->replica0, e->n_models))
        return fail(SGA_ERR_INVALID, std::string("sga_resample: ") + why);
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const int R = e->R, P = n_populations, N = R / P;
    const sga::ResampleScratch lay = sga::resample_scratch(R, P);
    HIPCHK(e->scratch[6].reserve(lay.bytes));
    unsigned char *s = static_cast<unsigned char *>(e->scratch[6].ptr);
    sga::ResampleArgs a{};
    a.energy = e->energy;
    a.best_energy = e->best_energy;
    a.C = reinterpret_cast<unsigned long long *>(s + lay.c);
    a.F = reinterpret_cast<int *>(s + lay.f);
    a.SP = reinterpret_cast<int *>(s + lay.sp);
    a.parent = reinterpret_cast<int32_t *>(s + lay.parent);
    a.take_best = reinterpret_cast<int *>(s + lay.take);
    a.shift = reinterpret_cast<double *>(s + lay.shift);
    a.sum = reinterpret_cast<unsigned long long *>(s + lay.sum);
    double *d_dbeta = reinterpret_cast<double *>(s + lay.dbeta);
    // (a pageable host array: the copy has left the caller's buffer when the call returns)
    HIPCHK(hipMemcpyAsync(d_dbeta, dbeta, (size_t)P * sizeof(double), hipMemcpyHostToDevice, st));
    a.dbeta = d_dbeta;
    a.N = N;
    a.n_pop = P;
    a.gpop0 = (uint32_t)(e->replica0 / N);
    a.seed_lo = (uint32_t)e->seed;
    a.seed_hi = (uint32_t)(e->seed >> 32);
    a.round = round;
    HIPCHK(sga::launch_resample_plan(a, st));
    HIPCHK(sga::launch_resample_copy(a.parent, a.take_best, e->spins, e->energy, e->best_spins, e->best_energy, e->sstride, R, st));
    e->fields_valid = false;  // (as after sga_set_spins: the next sweep seeds the cached fields again)
    bool wait = false;
    if (parents) {
        HIPCHK(hipMemcpyAsync(parents, a.parent, (size_t)R * sizeof(int32_t), hipMemcpyDefault, st));
        wait = wait || !is_device_ptr(parents);
    }
    if (shift) {
        HIPCHK(hipMemcpyAsync(shift, a.shift, (size_t)P * sizeof(double), hipMemcpyDefault, st));
        wait = wait || !is_device_ptr(shift);
    }
    if (weight_sum) {
        HIPCHK(hipMemcpyAsync(weight_sum, a.sum, (size_t)P * sizeof(uint64_t), hipMemcpyDefault, st));
        wait = wait || !is_device_ptr(weight_sum);
    }
    if (wait) HIPCHK(hipStreamSynchronize(st));
    return SGA_OK;
}

// ---- spin and link overlaps between pairs of replicas (pair_overlaps.hip) ----------------------
// Read only, under the rule of the replica observables above: a host pair list is staged in point_sites, host results
// leave through point_out (both grow-only), and nothing else of the engine is written.
namespace {
// nullptr where the engine's stored rows are ones the link walk serves (the cluster move's problems; the graph of
// sga_set_csr_shared is one, whatever the field vectors), else why not
const char *links_refusal(const sga_engine *e) {
    if (e->tsp) return "link overlaps are not implemented for sga_set_tsp problems (no stored rows to walk)";
    if (e->groups) return "link overlaps are not implemented for sga_set_groups / sga_set_groups_csr problems (no stored rows to walk)";
    if (e->ragged) return "link overlaps are not implemented for ragged CSR batches";
    if (!e->csr || !e->rowptr64 || !e->cv) return "link overlaps need sparse (CSR) couplings: dense couplings have no stored links";
    if (e->n > sga::PAIR_OVERLAP_MAX_N) return "link overlaps: the bitmap of n differing sites does not fit LDS (n / 8 bytes of 160 KiB)";
    return nullptr;
}
int link_group_log2(const sga_engine *e) { return sga::pair_overlap_group_log2(e->layout_entries, e->n); }
}  // namespace

int sga_get_link_count(sga_engine *e, int64_t *n_links) {
    if (!e || !n_links) return fail(SGA_ERR_INVALID, "NULL argument");
    if (const char *why = observables_ready(e)) return fail(SGA_ERR_INVALID, why);
    if (const char *why = links_refusal(e)) return fail(SGA_ERR_UNSUPPORTED, why);
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(e->point_out.reserve(sizeof(unsigned long long)));
    unsigned long long *d = static_cast<unsigned long long *>(e->point_out.ptr);
    HIPCHK(hipMemsetAsync(d, 0, sizeof(unsigned long long), e->stream));
    HIPCHK(sga::launch_link_count(e->rowptr64, e->cv, e->n, link_group_log2(e), d, e->stream));
    HIPCHK(hipMemcpyAsync(n_links, d, sizeof(int64_t), hipMemcpyDefault, e->stream));
    if (!is_device_ptr(n_links)) HIPCHK(hipStreamSynchronize(e->stream));
    return SGA_OK;
}

int sga_get_pair_overlaps(sga_engine *e, int which, const int32_t *pairs, int count, int32_t *dist, int64_t *broken) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (const char *why = observables_ready(e)) return fail(SGA_ERR_INVALID, why);
    if (!observed_which(which)) return fail(SGA_ERR_INVALID, "which must be SGA_SPINS_CURRENT or SGA_SPINS_BEST");
    if (!dist && !broken) return fail(SGA_ERR_INVALID, "dist and broken are both NULL");
    if (pairs && is_device_ptr(pairs)) return fail(SGA_ERR_INVALID, "pairs must be a host buffer");
    if (const char *why = sga::pair_overlap_pairs_check(pairs, count, e->R)) return fail(SGA_ERR_INVALID, why);
    if (broken)
        if (const char *why = links_refusal(e)) return fail(SGA_ERR_UNSUPPORTED, why);
    if (count == 0) return SGA_OK;
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const size_t cnt = (size_t)count;
    // (a pageable host list: the copy has left the caller's buffer when the call returns)
    HIPCHK(e->point_sites.reserve(2 * cnt * sizeof(int32_t)));
    HIPCHK(hipMemcpyAsync(e->point_sites.ptr, pairs, 2 * cnt * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const bool dist_host = dist && !is_device_ptr(dist), broken_host = broken && !is_device_ptr(broken);
    // host results: [count] int64 b, then [count] int32 d
    if (dist_host || broken_host) HIPCHK(e->point_out.reserve(cnt * (sizeof(int64_t) + sizeof(int32_t))));
    long long *stage_b = static_cast<long long *>(e->point_out.ptr);
    int32_t *stage_d = reinterpret_cast<int32_t *>(stage_b + cnt);
    sga::PairOverlapArgs a{};
    a.spins = observed_rows(e, which);
    a.pairs = static_cast<const int32_t *>(e->point_sites.ptr);
    a.dist = dist_host ? stage_d : dist;
    a.broken = broken_host ? stage_b : reinterpret_cast<long long *>(broken);
    a.links = broken ? 1 : 0;
    if (a.links) a.rowptr64 = e->rowptr64, a.cv = e->cv, a.group_log2 = link_group_log2(e);
    a.n = e->n, a.sstride = e->sstride, a.R = e->R, a.count = count, a.replica0 = e->replica0;
    HIPCHK(sga::launch_pair_overlaps(a, st));
    if (dist_host) HIPCHK(hipMemcpyAsync(dist, stage_d, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (broken_host) HIPCHK(hipMemcpyAsync(broken, stage_b, cnt * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (dist_host || broken_host) HIPCHK(hipStreamSynchronize(st));
    return SGA_OK;
}

int sga_accumulate_ladder_overlaps(sga_engine *e, int slot_lo, int slot_hi, uint64_t *hist_q, int bins_q, int q_shift,
                                   uint64_t *hist_l, int bins_l, int l_shift) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (const char *why = observables_ready(e)) return fail(SGA_ERR_INVALID, why);
    if (const char *why = sga::pair_overlap_hist_check(hist_q != nullptr, bins_q, q_shift, hist_l != nullptr, bins_l, l_shift))
        return fail(SGA_ERR_INVALID, why);
    if (!is_device_ptr(hist_q) || (hist_l && !is_device_ptr(hist_l)))
        return fail(SGA_ERR_INVALID, "the histograms must be device buffers (they stay on the device for the whole run)");
    if (e->n_ladders <= 0 || !e->slot_to_rep) return fail(SGA_ERR_INVALID, "no ladder (call sga_set_ladder)");
    if (e->n_ladders % 2 != 0) return fail(SGA_ERR_INVALID, "overlaps between ladders need an even number of ladders");
    if (e->R != e->Rg) return fail(SGA_ERR_INVALID, "overlaps between ladders need every replica on this rank (R_local == R_global)");
    const int L = e->Rg / e->n_ladders;
    if (slot_lo < 0 || slot_hi > L || slot_lo > slot_hi) return fail(SGA_ERR_INVALID, "slot range outside [0, slots)");
    if (hist_l)
        if (const char *why = links_refusal(e)) return fail(SGA_ERR_UNSUPPORTED, why);
    if (slot_lo == slot_hi) return SGA_OK;
    HIPCHK(hipSetDevice(e->device));
    sga::PairOverlapArgs a{};
    a.spins = e->spins;
    a.slot_to_rep = e->slot_to_rep;
    a.L = L, a.slot_lo = slot_lo, a.n_slots = slot_hi - slot_lo;
    a.hist_q = reinterpret_cast<unsigned long long *>(hist_q);
    a.hist_l = reinterpret_cast<unsigned long long *>(hist_l);
    a.bins_q = bins_q, a.q_shift = q_shift, a.bins_l = hist_l ? bins_l : 1, a.l_shift = hist_l ? l_shift : 0;
    a.links = hist_l ? 1 : 0;
    if (a.links) a.rowptr64 = e->rowptr64, a.cv = e->cv, a.group_log2 = link_group_log2(e);
    a.n = e->n, a.sstride = e->sstride, a.R = e->R, a.count = (e->n_ladders / 2) * a.n_slots, a.replica0 = e->replica0;
    HIPCHK(sga::launch_pair_overlaps(a, e->stream));
    return SGA_OK;
}

// ---- class-resolved overlaps between pairs of replicas (class_overlaps.hip) -------------------
// Read only, under the same rule: a host pair list and behind it a host class map are staged in point_sites, a host
// result leaves through point_out (both grow-only), and nothing else of the engine is written.
int sga_get_class_overlaps(sga_engine *e, int which, const int32_t *pairs, int count, const int32_t *classes, int64_t ld,
                           int n_maps, int n_classes, int32_t *dist) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (const char *why = observables_ready(e)) return fail(SGA_ERR_INVALID, why);
    if (!observed_which(which)) return fail(SGA_ERR_INVALID, "which must be SGA_SPINS_CURRENT or SGA_SPINS_BEST");
    if (pairs && is_device_ptr(pairs)) return fail(SGA_ERR_INVALID, "pairs must be a host buffer");
    if (const char *why = sga::pair_overlap_pairs_check(pairs, count, e->R)) return fail(SGA_ERR_INVALID, why);
    if (const char *why = sga::class_overlap_args_check(classes != nullptr, dist != nullptr, n_maps, n_classes, ld, e->n))
        return fail(SGA_ERR_INVALID, why);
    if (const char *why = sga::class_overlap_unsupported(n_maps, n_classes)) return fail(SGA_ERR_UNSUPPORTED, why);
    if (count == 0) return SGA_OK;
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const size_t cnt = (size_t)count, mc = (size_t)n_maps * (size_t)n_classes, n = (size_t)e->n;
    const bool map_host = !is_device_ptr(classes), dist_host = !is_device_ptr(dist);
    // the pair list, then a host map packed to ld = n rounded up to 4 (pageable host buffers: the copies have left them on return)
    const size_t pair_bytes = (2 * cnt * sizeof(int32_t) + 15) / 16 * 16;
    const size_t ld4 = (n + 3) / 4 * 4;  // (rows of the staged map start 16-byte aligned: the kernel loads int4)
    HIPCHK(e->point_sites.reserve(pair_bytes + (map_host ? (size_t)n_maps * ld4 * sizeof(int32_t) : 0)));
    unsigned char *stage = static_cast<unsigned char *>(e->point_sites.ptr);
    HIPCHK(hipMemcpyAsync(stage, pairs, 2 * cnt * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (map_host)
        HIPCHK(hipMemcpy2DAsync(stage + pair_bytes, ld4 * sizeof(int32_t), classes, (size_t)ld * sizeof(int32_t), n * sizeof(int32_t),
                                (size_t)n_maps, hipMemcpyHostToDevice, st));
    if (dist_host) HIPCHK(e->point_out.reserve(cnt * mc * sizeof(int32_t)));
    sga::ClassOverlapArgs a{};
    a.spins = observed_rows(e, which);
    a.pairs = reinterpret_cast<const int32_t *>(stage);
    a.classes = map_host ? reinterpret_cast<const int32_t *>(stage + pair_bytes) : classes;
    a.ld = map_host ? (long long)ld4 : (long long)ld;
    a.n_maps = n_maps, a.n_classes = n_classes;
    a.dist = dist_host ? static_cast<int32_t *>(e->point_out.ptr) : dist;
    a.n = e->n, a.sstride = e->sstride, a.R = e->R, a.count = count, a.replica0 = e->replica0;
    HIPCHK(sga::launch_class_overlaps(a, st));
    if (dist_host) {
        HIPCHK(hipMemcpyAsync(dist, a.dist, cnt * mc * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return SGA_OK;
}

int sga_accumulate_ladder_class_overlaps(sga_engine *e, int slot_lo, int slot_hi, const int32_t *classes, int64_t ld, int n_maps,
                                         int n_classes, uint64_t *sum1, uint64_t *sum2) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (const char *why = observables_ready(e)) return fail(SGA_ERR_INVALID, why);
    if (const char *why = sga::class_overlap_args_check(classes != nullptr, sum1 != nullptr, n_maps, n_classes, ld, e->n))
        return fail(SGA_ERR_INVALID, why);
    if (!is_device_ptr(classes) || !is_device_ptr(sum1) || (sum2 && !is_device_ptr(sum2)))
        return fail(SGA_ERR_INVALID, "classes, sum1 and sum2 must be device buffers (they stay on the device for the whole run)");
    if (e->n_ladders <= 0 || !e->slot_to_rep) return fail(SGA_ERR_INVALID, "no ladder (call sga_set_ladder)");
    if (e->n_ladders % 2 != 0) return fail(SGA_ERR_INVALID, "overlaps between ladders need an even number of ladders");
    if (e->R != e->Rg) return fail(SGA_ERR_INVALID, "overlaps between ladders need every replica on this rank (R_local == R_global)");
    const int L = e->Rg / e->n_ladders;
    if (slot_lo < 0 || slot_hi > L || slot_lo > slot_hi) return fail(SGA_ERR_INVALID, "slot range outside [0, slots)");
    if (const char *why = sga::class_overlap_unsupported(n_maps, n_classes)) return fail(SGA_ERR_UNSUPPORTED, why);
    if (slot_lo == slot_hi) return SGA_OK;
    HIPCHK(hipSetDevice(e->device));
    sga::ClassOverlapArgs a{};
    a.spins = e->spins;
    a.slot_to_rep = e->slot_to_rep;
    a.L = L, a.slot_lo = slot_lo, a.n_slots = slot_hi - slot_lo;
    a.classes = classes, a.ld = (long long)ld, a.n_maps = n_maps, a.n_classes = n_classes;
    a.sum1 = reinterpret_cast<unsigned long long *>(sum1);
    a.sum2 = reinterpret_cast<unsigned long long *>(sum2);
    a.n = e->n, a.sstride = e->sstride, a.R = e->R, a.count = (e->n_ladders / 2) * a.n_slots, a.replica0 = e->replica0;
    HIPCHK(sga::launch_class_overlaps(a, e->stream));
    return SGA_OK;
}

int sga_get_route_query(sga_engine *e, sga_route_query *out) {
    if (!e || !out) return fail(SGA_ERR_INVALID, "NULL argument");
    if (e->n <= 0) return fail(SGA_ERR_INVALID, "no couplings set");
    *out = route_query_of(e);
    return SGA_OK;
}

int sga_get_last_kernel(sga_engine *e, char *buf, int buflen) {
    if (!e || !buf || buflen <= 0) return fail(SGA_ERR_INVALID, "bad arguments");
    std::snprintf(buf, (size_t)buflen, "%s", e->last_kernel);
    return SGA_OK;
}

int sga_last_kernel(char *buf, int buflen) {
    if (!buf || buflen <= 0) return fail(SGA_ERR_INVALID, "bad arguments");
    std::snprintf(buf, (size_t)buflen, "%s", sga::last_sweep_kernel());
    return SGA_OK;
}

}  // extern "C"
