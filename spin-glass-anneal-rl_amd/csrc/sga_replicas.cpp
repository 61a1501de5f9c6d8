// sga_replicas.cpp -- measurements and moves over the replicas, the engine half (the pure half: sga_replicas.h).  None
// keeps state of its own.  A host list reaches the device through stage_host, a result leaves through DevOut / deliver
// (sga_engine_impl.h): the kernels write the caller's device buffer itself, a host buffer's result goes through a
// grow-only slot and is waited for -- so the steady-state call allocates nothing.
#include "sga_engine_impl.h"

namespace {
const int8_t *observed_rows(const sga_engine *e, int which) { return which == SGA_SPINS_BEST ? e->best_spins : e->spins; }
bool observed_which(int which) { return which == SGA_SPINS_CURRENT || which == SGA_SPINS_BEST; }
const char *observables_ready(const sga_engine *e) {
    if (e->n <= 0) return "no couplings set";
    if (e->R <= 0 || !e->spins || !e->best_spins) return "no replicas";
    return nullptr;
}
// The ladder form of a pair record (ClusterArgs, PairOverlapArgs, ClassOverlapArgs): ladders 2c and 2c + 1, slots
// [slot_lo, slot_hi); the pairs it names.
template <typename Args>
int ladder_pairs_into(Args &a, const sga_engine *e, int L, int slot_lo, int slot_hi) {
    a.slot_to_rep = e->slot_to_rep;
    a.L = L, a.slot_lo = slot_lo, a.n_slots = slot_hi - slot_lo;
    return (e->n_ladders / 2) * a.n_slots;
}

// ---- replica observables (observables.hip) --------------------------------------------------
// Read only: the result of a host `out` goes through the point_out slot, a host `cfg` through point_sites, and nothing
// else of the engine is written -- not the spins, fields, counters, bests, window plan or last_kernel.
// out[a * ldq + b] = sum_{i < n} A_a[i] B_b[i], A the local replicas' rows; B on the device.  Every argument is checked
// by the caller; the work goes on the engine's stream, and a host `out` is waited for.
int observables_product(sga_engine *e, const int8_t *A, const int8_t *B, long long ldb, int rows_b, bool symmetric,
                        int32_t *out, int64_t ldq) {
    sga::ObservablesArgs a{};
    a.A = A, a.B = B, a.lda = e->sstride, a.ldb = ldb;
    a.rows_a = e->R, a.rows_b = rows_b, a.n = e->n, a.symmetric = symmetric ? 1 : 0;
    a.plan = sga::observables_plan(e->n, e->R, rows_b, e->cus);
    DevOut<int32_t> q(out, (size_t)rows_b, (size_t)e->R, (size_t)ldq);
    if (const int rc = q.direct(e->point_out)) return rc;
    a.out = q.ptr, a.ldq = (long long)q.ld();
    if (a.plan.ksplit > 1)  // the K ranges add into the result
        HIPCHK(hipMemset2DAsync(a.out, (size_t)a.ldq * sizeof(int32_t), 0, (size_t)rows_b * sizeof(int32_t), (size_t)e->R, e->stream));
    HIPCHK(sga::launch_observables_product(a, e->stream));
    return deliver(e->stream, q);
}
}  // namespace

int sga_get_magnetizations(sga_engine *e, int which, int32_t *out) {
    if (!e || !out) return fail(SGA_ERR_INVALID, "NULL argument");
    if (const char *why = observables_ready(e)) return fail(SGA_ERR_INVALID, why);
    if (!observed_which(which)) return fail(SGA_ERR_INVALID, "which must be SGA_SPINS_CURRENT or SGA_SPINS_BEST");
    HIPCHK(hipSetDevice(e->device));
    DevOut<int32_t> m(out, (size_t)e->R);
    if (const int rc = m.direct(e->point_out)) return rc;
    HIPCHK(sga::launch_observables_row_sums(observed_rows(e, which), e->sstride, e->n, e->R, m.ptr, e->stream));
    return deliver(e->stream, m);
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
        if (const int rc = stage_host(e->point_sites, (size_t)count * (size_t)ldb, 0, cfg, (size_t)e->n, e->stream, (size_t)count,
                                      (size_t)ld, (size_t)ldb))
            return rc;
        B = slot_at<const int8_t>(e->point_sites);
    }
    return observables_product(e, observed_rows(e, which), B, ldb, count, false, out, ldq);
}

// ---- isoenergetic cluster moves (cluster_moves.hip) ------------------------------------------
// A host pair list is staged in scratch slot 7 (as sga_exchange_pairs stages its list), the energies before the move
// and the touched flags lie in slot 6, a host `sizes` goes through point_out.
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
    DevOut<int32_t> out(sizes, (size_t)count);
    if (const int rc = out.direct(e->point_out)) return rc;
    HIPCHK(hipMemcpyAsync(saved, e->energy, R * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemsetAsync(touched, 0, R * sizeof(int), st));
    a.spins = e->spins, a.rowptr64 = e->rowptr64, a.cv = e->cv, a.n_accepted = e->n_acc;
    a.sizes = out.ptr, a.touched = touched;
    geometry_into(a, e);
    seed_into(a, e);
    a.count = count, a.round = round;
    HIPCHK(sga::launch_cluster_moves(a, st));
    e->fields_valid = false;
    // the whole range, as sga_recompute_energies forms it: the same pass, so the same bits; the replicas whose spins did
    // not change get their energies back
    if (const int rc = recompute_energy_range(e, 0, e->R)) return rc;
    HIPCHK(sga::launch_cluster_finish(touched, saved, e->energy, e->spins, e->best_energy, e->best_spins, e->sstride, e->R, st));
    return deliver(st, out);
}
}  // namespace

int sga_cluster_move_pairs(sga_engine *e, const int32_t *pairs, int count, uint32_t round, int32_t *sizes) {
    if (!e || !pairs) return fail(SGA_ERR_INVALID, "NULL argument");
    int code = SGA_OK;
    if (const char *why = cluster_refusal(e, &code)) return fail(code, why);
    if (count < 0) return fail(SGA_ERR_INVALID, "count is negative");
    if (const int rc = refuse_device_ptr(pairs, "pairs")) return rc;
    std::vector<unsigned char> seen((size_t)e->R);
    const int reps_per_model = e->shared_j && e->n_models > 1 ? e->Rg / e->n_models : 0;
    if (const char *why = sga::cluster_pairs_check(pairs, count, e->R, e->replica0, reps_per_model, seen.data()))
        return fail(SGA_ERR_INVALID, why);
    if (count == 0) return SGA_OK;
    HIPCHK(hipSetDevice(e->device));
    const size_t bytes = (size_t)2 * count * sizeof(int32_t);
    if (const int rc = stage_host(e->scratch[7], bytes, 0, pairs, bytes, e->stream)) return rc;
    sga::ClusterArgs a{};
    a.pairs = slot_at<const int32_t>(e->scratch[7]);
    return cluster_move_run(e, a, count, round, sizes);
}

int sga_cluster_move_ladders(sga_engine *e, int slot_lo, int slot_hi, uint32_t round, int32_t *sizes) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    int code = SGA_OK;
    if (const char *why = cluster_refusal(e, &code)) return fail(code, why);
    const sga::LadderPairs lp = sga::ladder_pairs_check(e->n_ladders, e->slot_to_rep != nullptr, e->R, e->Rg, slot_lo, slot_hi, "cluster moves");
    if (lp.why) return fail(SGA_ERR_INVALID, lp.why);
    if (e->shared_j && e->n_models > 1) {  // a ladder's slots hold its own L replicas: both ladders under one field vector
        const int reps = e->Rg / e->n_models;
        for (int c = 0; c < e->n_ladders / 2; ++c)
            if ((2 * c * lp.L) / reps != ((2 * c + 2) * lp.L - 1) / reps)
                return fail(SGA_ERR_INVALID, "shared-coupling CSR batch: ladders " + std::to_string(2 * c) + " and " +
                                                 std::to_string(2 * c + 1) + " lie under two models (their field vectors differ)");
    }
    if (slot_lo == slot_hi) return SGA_OK;
    HIPCHK(hipSetDevice(e->device));
    sga::ClusterArgs a{};
    const int count = ladder_pairs_into(a, e, lp.L, slot_lo, slot_hi);
    return cluster_move_run(e, a, count, round, sizes);
}

// ---- population annealing: the resampling step (resample.hip) ---------------------------------
// The plan's arrays (sga_replicas.h, resample_scratch) lie in scratch slot 6 with the staged dbeta behind them, the
// outputs leave from there; the two kernels follow each other on the engine's stream.
int sga_resample(sga_engine *e, int n_populations, const double *dbeta, uint32_t round, int32_t *parents, double *shift,
                 uint64_t *weight_sum) {
    if (!e || !dbeta) return fail(SGA_ERR_INVALID, "NULL argument");
    if (const char *why = observables_ready(e)) return fail(SGA_ERR_INVALID, why);
    if (const int rc = refuse_device_ptr(dbeta, "dbeta")) return rc;
    if (const char *why = sga::resample_check(n_populations, dbeta, e->R, e->Rg, e->replica0, e->n_models))
        return fail(SGA_ERR_INVALID, std::string("sga_resample: ") + why);
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const int R = e->R, P = n_populations, N = R / P;
    const sga::ResampleScratch lay = sga::resample_scratch(R, P);
    if (const int rc = stage_host(e->scratch[6], lay.bytes, lay.dbeta, dbeta, (size_t)P * sizeof(double), st)) return rc;
    const Scratch &s = e->scratch[6];
    DevOut<int32_t> out_parents(parents, (size_t)R);
    DevOut<double> out_shift(shift, (size_t)P);
    DevOut<uint64_t> out_sum(weight_sum, (size_t)P);
    out_parents.staged(slot_at<void>(s, lay.parent)), out_shift.staged(slot_at<void>(s, lay.shift)), out_sum.staged(slot_at<void>(s, lay.sum));
    sga::ResampleArgs a{};
    a.energy = e->energy, a.best_energy = e->best_energy, a.dbeta = slot_at<const double>(s, lay.dbeta);
    a.C = slot_at<unsigned long long>(s, lay.c), a.F = slot_at<int>(s, lay.f), a.SP = slot_at<int>(s, lay.sp);
    a.parent = out_parents.ptr, a.take_best = slot_at<int>(s, lay.take);
    a.shift = out_shift.ptr, a.sum = reinterpret_cast<unsigned long long *>(out_sum.ptr);
    a.N = N, a.n_pop = P, a.gpop0 = (uint32_t)(e->replica0 / N), a.round = round;
    seed_into(a, e);
    HIPCHK(sga::launch_resample_plan(a, st));
    HIPCHK(sga::launch_resample_copy(a.parent, a.take_best, e->spins, e->energy, e->best_spins, e->best_energy, e->sstride, R, st));
    e->fields_valid = false;  // (as after sga_set_spins: the next sweep seeds the cached fields again)
    return deliver(st, out_parents, out_shift, out_sum);
}

// ---- spin and link overlaps between pairs of replicas (pair_overlaps.hip) ----------------------
// Read only, under the rule of the replica observables above: a host pair list is staged in point_sites, host results
// leave through point_out, and nothing else of the engine is written.
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
void links_into(sga::PairOverlapArgs &a, const sga_engine *e, bool links) {
    a.links = links ? 1 : 0;
    if (links) a.rowptr64 = e->rowptr64, a.cv = e->cv, a.group_log2 = sga::pair_overlap_group_log2(e->layout_entries, e->n);
}
}  // namespace

int sga_get_link_count(sga_engine *e, int64_t *n_links) {
    if (!e || !n_links) return fail(SGA_ERR_INVALID, "NULL argument");
    if (const char *why = observables_ready(e)) return fail(SGA_ERR_INVALID, why);
    if (const char *why = links_refusal(e)) return fail(SGA_ERR_UNSUPPORTED, why);
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(e->point_out.reserve(sizeof(unsigned long long)));
    DevOut<int64_t> out(n_links, 1);
    out.staged(e->point_out.ptr);
    HIPCHK(hipMemsetAsync(out.ptr, 0, sizeof(unsigned long long), e->stream));
    HIPCHK(sga::launch_link_count(e->rowptr64, e->cv, e->n, sga::pair_overlap_group_log2(e->layout_entries, e->n),
                                  reinterpret_cast<unsigned long long *>(out.ptr), e->stream));
    return deliver(e->stream, out);
}

int sga_get_pair_overlaps(sga_engine *e, int which, const int32_t *pairs, int count, int32_t *dist, int64_t *broken) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (const char *why = observables_ready(e)) return fail(SGA_ERR_INVALID, why);
    if (!observed_which(which)) return fail(SGA_ERR_INVALID, "which must be SGA_SPINS_CURRENT or SGA_SPINS_BEST");
    if (!dist && !broken) return fail(SGA_ERR_INVALID, "dist and broken are both NULL");
    if (const int rc = refuse_device_ptr(pairs, "pairs")) return rc;
    if (const char *why = sga::pair_overlap_pairs_check(pairs, count, e->R)) return fail(SGA_ERR_INVALID, why);
    if (broken)
        if (const char *why = links_refusal(e)) return fail(SGA_ERR_UNSUPPORTED, why);
    if (count == 0) return SGA_OK;
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const size_t cnt = (size_t)count;
    if (const int rc = stage_host(e->point_sites, 2 * cnt * sizeof(int32_t), 0, pairs, 2 * cnt * sizeof(int32_t), st)) return rc;
    // host results: [count] int64 b, then [count] int32 d
    DevOut<int32_t> out_d(dist, cnt);
    DevOut<int64_t> out_b(broken, cnt);
    if (out_d.host || out_b.host) HIPCHK(e->point_out.reserve(cnt * (sizeof(int64_t) + sizeof(int32_t))));
    out_b.direct(slot_at<void>(e->point_out));
    out_d.direct(slot_at<void>(e->point_out, cnt * sizeof(int64_t)));
    sga::PairOverlapArgs a{};
    a.spins = observed_rows(e, which), a.pairs = slot_at<const int32_t>(e->point_sites);
    a.dist = out_d.ptr, a.broken = reinterpret_cast<long long *>(out_b.ptr);
    links_into(a, e, broken != nullptr);
    geometry_into(a, e);
    a.count = count;
    HIPCHK(sga::launch_pair_overlaps(a, st));
    return deliver(st, out_d, out_b);
}

int sga_accumulate_ladder_overlaps(sga_engine *e, int slot_lo, int slot_hi, uint64_t *hist_q, int bins_q, int q_shift,
                                   uint64_t *hist_l, int bins_l, int l_shift) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (const char *why = observables_ready(e)) return fail(SGA_ERR_INVALID, why);
    if (const char *why = sga::pair_overlap_hist_check(hist_q != nullptr, bins_q, q_shift, hist_l != nullptr, bins_l, l_shift))
        return fail(SGA_ERR_INVALID, why);
    if (!is_device_ptr(hist_q) || (hist_l && !is_device_ptr(hist_l)))
        return fail(SGA_ERR_INVALID, "the histograms must be device buffers (they stay on the device for the whole run)");
    const sga::LadderPairs lp = sga::ladder_pairs_check(e->n_ladders, e->slot_to_rep != nullptr, e->R, e->Rg, slot_lo, slot_hi, "overlaps");
    if (lp.why) return fail(SGA_ERR_INVALID, lp.why);
    if (hist_l)
        if (const char *why = links_refusal(e)) return fail(SGA_ERR_UNSUPPORTED, why);
    if (slot_lo == slot_hi) return SGA_OK;
    HIPCHK(hipSetDevice(e->device));
    sga::PairOverlapArgs a{};
    a.spins = e->spins;
    a.hist_q = reinterpret_cast<unsigned long long *>(hist_q), a.hist_l = reinterpret_cast<unsigned long long *>(hist_l);
    a.bins_q = bins_q, a.q_shift = q_shift, a.bins_l = hist_l ? bins_l : 1, a.l_shift = hist_l ? l_shift : 0;
    links_into(a, e, hist_l != nullptr);
    geometry_into(a, e);
    a.count = ladder_pairs_into(a, e, lp.L, slot_lo, slot_hi);
    HIPCHK(sga::launch_pair_overlaps(a, e->stream));
    return SGA_OK;
}

// ---- class-resolved overlaps between pairs of replicas (class_overlaps.hip) -------------------
// Read only, under the same rule: a host pair list and behind it a host class map are staged in point_sites, a host
// result leaves through point_out, and nothing else of the engine is written.
int sga_get_class_overlaps(sga_engine *e, int which, const int32_t *pairs, int count, const int32_t *classes, int64_t ld,
                           int n_maps, int n_classes, int32_t *dist) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (const char *why = observables_ready(e)) return fail(SGA_ERR_INVALID, why);
    if (!observed_which(which)) return fail(SGA_ERR_INVALID, "which must be SGA_SPINS_CURRENT or SGA_SPINS_BEST");
    if (const int rc = refuse_device_ptr(pairs, "pairs")) return rc;
    if (const char *why = sga::pair_overlap_pairs_check(pairs, count, e->R)) return fail(SGA_ERR_INVALID, why);
    if (const char *why = sga::class_overlap_args_check(classes != nullptr, dist != nullptr, n_maps, n_classes, ld, e->n))
        return fail(SGA_ERR_INVALID, why);
    if (const char *why = sga::class_overlap_unsupported(n_maps, n_classes)) return fail(SGA_ERR_UNSUPPORTED, why);
    if (count == 0) return SGA_OK;
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const size_t cnt = (size_t)count, mc = (size_t)n_maps * (size_t)n_classes, n = (size_t)e->n;
    const bool map_host = !is_device_ptr(classes);
    // the pair list, then a host map packed to ld = n rounded up to 4
    const size_t pair_bytes = (2 * cnt * sizeof(int32_t) + 15) / 16 * 16;
    const size_t ld4 = (n + 3) / 4 * 4;  // (rows of the staged map start 16-byte aligned: the kernel loads int4)
    const size_t total = pair_bytes + (map_host ? (size_t)n_maps * ld4 * sizeof(int32_t) : 0);
    if (const int rc = stage_host(e->point_sites, total, 0, pairs, 2 * cnt * sizeof(int32_t), st)) return rc;
    if (map_host)
        if (const int rc = stage_host(e->point_sites, total, pair_bytes, classes, n * sizeof(int32_t), st, (size_t)n_maps,
                                      (size_t)ld * sizeof(int32_t), ld4 * sizeof(int32_t)))
            return rc;
    DevOut<int32_t> out(dist, cnt * mc);
    if (const int rc = out.direct(e->point_out)) return rc;
    sga::ClassOverlapArgs a{};
    a.spins = observed_rows(e, which), a.pairs = slot_at<const int32_t>(e->point_sites), a.dist = out.ptr;
    a.classes = map_host ? slot_at<const int32_t>(e->point_sites, pair_bytes) : classes;
    a.ld = map_host ? (long long)ld4 : (long long)ld, a.n_maps = n_maps, a.n_classes = n_classes;
    geometry_into(a, e);
    a.count = count;
    HIPCHK(sga::launch_class_overlaps(a, st));
    return deliver(st, out);
}

int sga_accumulate_ladder_class_overlaps(sga_engine *e, int slot_lo, int slot_hi, const int32_t *classes, int64_t ld, int n_maps,
                                         int n_classes, uint64_t *sum1, uint64_t *sum2) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (const char *why = observables_ready(e)) return fail(SGA_ERR_INVALID, why);
    if (const char *why = sga::class_overlap_args_check(classes != nullptr, sum1 != nullptr, n_maps, n_classes, ld, e->n))
        return fail(SGA_ERR_INVALID, why);
    if (!is_device_ptr(classes) || !is_device_ptr(sum1) || (sum2 && !is_device_ptr(sum2)))
        return fail(SGA_ERR_INVALID, "classes, sum1 and sum2 must be device buffers (they stay on the device for the whole run)");
    const sga::LadderPairs lp = sga::ladder_pairs_check(e->n_ladders, e->slot_to_rep != nullptr, e->R, e->Rg, slot_lo, slot_hi, "overlaps");
    if (lp.why) return fail(SGA_ERR_INVALID, lp.why);
    if (const char *why = sga::class_overlap_unsupported(n_maps, n_classes)) return fail(SGA_ERR_UNSUPPORTED, why);
    if (slot_lo == slot_hi) return SGA_OK;
    HIPCHK(hipSetDevice(e->device));
    sga::ClassOverlapArgs a{};
    a.spins = e->spins, a.classes = classes, a.ld = (long long)ld, a.n_maps = n_maps, a.n_classes = n_classes;
    a.sum1 = reinterpret_cast<unsigned long long *>(sum1), a.sum2 = reinterpret_cast<unsigned long long *>(sum2);
    geometry_into(a, e);
    a.count = ladder_pairs_into(a, e, lp.L, slot_lo, slot_hi);
    HIPCHK(sga::launch_class_overlaps(a, e->stream));
    return SGA_OK;
}
