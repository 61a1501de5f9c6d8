// sga_engine_impl.h -- what the translation units of the host side share: the engine record, the error / option
// plumbing and the helpers several of them call.  Internal to libsga.so; the ABI is include/sga.h.
//   sga_engine.cpp    handle, options, replicas, ladder, sweeps, single-site operators, exchange
//   sga_problem.cpp   sga_set_dense / sga_set_csr / sga_set_tsp: scans, packing, CSR layouts
//   sga_autotune.cpp  sga_autotune (measured launch geometry / sweep form)
//   sga_state.cpp     state access, checkpoint / resume, timing, sga_describe, checksum, route query
//   sga_replicas.cpp  measurements and moves over the replicas: observables, cluster moves, resampling, pair and class
//                     overlaps over the pure half (sga_replicas.h: plans, argument records, the checks of the lists)
//   sga_route.cpp     WHICH form runs: pure functions of the problem's traits and the options, and the cached-field
//                     modes' sweep-time policy over the acceptance counters (no HIP calls)
//   sga_classify.cpp  WHICH arithmetic a problem admits: accumulation class, accept table, cached-field eligibility and
//                     the refusal reasons, pure functions of the set-time scan summaries (no HIP calls)
//   sga_windows.cpp   the window forms of the dense sweep (row-shared, its tiles, sequential): admission as pure functions
//                     of WindowTraits, the forms' state by lifetime (WindowState), their scratch and per-call plan
//   sga_quantum.cpp   simulated quantum annealing: the two transverse sweeps, the world-line clusters and the exchange along
//                     the transverse field over the pure half (sga_quantum.h: slice geometry, admission rules)
// The engine record is split by lifetime.  sga_engine derives from ProblemState (what the next sga_set_* must not see)
// and ReplicaState (what the next sga_init_replicas must not see), so every member is still e->member; what survives
// both stays in sga_engine itself.  A sub-record's defaults stand once, in its declaration: its reset releases the
// device buffers it owns -- the one list there is -- and assigns a fresh record.  tests/c_abi/engine_record.cpp runs
// the resets over a filled engine without a GPU.
#ifndef SGA_ENGINE_IMPL_H
#define SGA_ENGINE_IMPL_H
#include <hip/hip_runtime.h>
#include <algorithm>
#include <functional>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>
#include "sga.h"
#include "sga_kernels.h"
#include "sga_quantum.h"
#include "sga_replicas.h"
#include "sga_route.h"
#include "sga_windows.h"

namespace sga_impl {


#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return fail(_e == hipErrorOutOfMemory ? SGA_ERR_MEMORY : SGA_ERR_DEVICE,       \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                \
    } while (0)

template <typename T>
void dev_free(T *&p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}
// What a reset hands the device buffers it drops to: the engine hipFree, tests/c_abi/engine_record.cpp a recorder.
using Release = sga_windows::WindowState::Release;
inline void dev_release(void *p) { (void)hipFree(p); }
inline void release_all(std::initializer_list<void *> owned, Release release) {
    for (void *p : owned)
        if (p) release(p);
}

inline bool is_device_ptr(const void *p) {
    if (!p) return false;
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // clear: plain host memory
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

// Grow-only device scratch slots owned by an engine: staging of host-side call arguments and
// outputs re-uses them, so the steady-state call path performs no hipMalloc / hipFree (which
// would synchronise the device).
struct Scratch {
    void *ptr = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 2 + 256;
        hipError_t e = hipMalloc(&ptr, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

// A caller's HOST array into a scratch slot, `at` bytes from its base: the slot grows to `total` bytes (what lies in front
// of the copy and behind it is the caller's to lay out), one copy on `st`.  src_pitch > 0: `rows` rows of `bytes` bytes,
// taken src_pitch bytes apart and laid down dst_pitch apart.  (Pageable: the copy has left the buffer on return.)
inline int stage_host(Scratch &slot, size_t total, size_t at, const void *host, size_t bytes, hipStream_t st, size_t rows = 1,
                      size_t src_pitch = 0, size_t dst_pitch = 0) {
    HIPCHK(slot.reserve(total));
    unsigned char *dst = static_cast<unsigned char *>(slot.ptr) + at;
    if (src_pitch)
        HIPCHK(hipMemcpy2DAsync(dst, dst_pitch, host, src_pitch, bytes, rows, hipMemcpyHostToDevice, st));
    else
        HIPCHK(hipMemcpyAsync(dst, host, bytes, hipMemcpyHostToDevice, st));
    return SGA_OK;
}

// A read-only view of a user buffer on the device: borrowed if it already lives there,
// otherwise staged into a scratch slot.
template <typename T>
struct DevIn {
    const T *ptr = nullptr;
    bool staged = false;
    int init(Scratch &slot, const T *user, size_t count, hipStream_t st) {
        if (!user || count == 0) return SGA_OK;
        if (is_device_ptr(user)) {
            ptr = user;
            return SGA_OK;
        }
        if (const int rc = stage_host(slot, count * sizeof(T), 0, user, count * sizeof(T), st)) return rc;
        ptr = static_cast<const T *>(slot.ptr);
        staged = true;
        return SGA_OK;
    }
};

template <typename T>
inline T *slot_at(const Scratch &slot, size_t at = 0) { return reinterpret_cast<T *>(static_cast<unsigned char *>(slot.ptr) + at); }
inline int refuse_device_ptr(const void *p, const char *name) {
    return p && is_device_ptr(p) ? fail(SGA_ERR_INVALID, std::string(name) + " must be a host buffer") : SGA_OK;
}

// A result on its way to a user buffer, on the host or on the device.  ptr is what the kernels write (null: not asked
// for); deliver() queues the copies of a call's results and waits once where one lands on the host.  It is placed by
//   init    always through the slot, zero filled (the traces of sga_sweep, which waits itself)
//   direct  the caller's own buffer where that lies on the device, else the slot (or a place in one the caller reserved)
//   staged  a place in a slot whatever the caller's buffer is -- and whether or not it is asked for: the kernels write it
// rows > 0: a 2-D result, `rows` rows of `count` elements, the caller's `pitch` elements apart and the slot's packed.
// sum_on_host (the caller has refused a device buffer): the copy lands in `landed`, deliver() adds it to the caller's array.
template <typename T>
struct DevOut {
    T *ptr = nullptr, *user = nullptr;
    size_t count = 0, rows = 0, pitch = 0;
    bool host = false;    // the caller's buffer is known to lie on the host: the copy is waited for
    bool copied = false;  // ptr is not the caller's buffer
    bool summed = false;
    std::vector<T> landed;
    DevOut() = default;
    DevOut(T *user_, size_t count_, size_t rows_ = 0, size_t pitch_ = 0, bool sum_on_host = false)
        : user(user_), count(count_), rows(rows_), pitch(pitch_), host(user_ && (sum_on_host || !is_device_ptr(user_))),
          summed(user_ && sum_on_host) {}
    size_t bytes() const { return (rows ? rows : 1) * count * sizeof(T); }
    size_t ld() const { return copied ? count : pitch; }  // of ptr, in elements (2-D)
    int init(Scratch &slot, T *user_, size_t count_, hipStream_t st) {
        user = user_, count = count_;
        if (!user || count == 0) return SGA_OK;
        HIPCHK(slot.reserve(count * sizeof(T)));
        staged(slot.ptr);
        HIPCHK(hipMemsetAsync(ptr, 0, count * sizeof(T), st));
        return SGA_OK;
    }
    void direct(void *where) { copied = host, ptr = host ? static_cast<T *>(where) : user; }
    int direct(Scratch &slot) {
        if (host) HIPCHK(slot.reserve(bytes()));
        direct(slot.ptr);
        return SGA_OK;
    }
    void staged(void *where) { ptr = static_cast<T *>(where), copied = user != nullptr; }
    int flush(hipStream_t st) {
        if (!copied) return SGA_OK;
        const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDefault;
        if (summed) landed.resize(count);
        T *to = summed ? landed.data() : user;
        if (rows)
            HIPCHK(hipMemcpy2DAsync(to, pitch * sizeof(T), ptr, count * sizeof(T), count * sizeof(T), rows, kind, st));
        else
            HIPCHK(hipMemcpyAsync(to, ptr, count * sizeof(T), kind, st));
        return SGA_OK;
    }
    void land() { for (size_t i = 0; i < landed.size(); ++i) user[i] += landed[i]; }
};
// The end of a call: the copies of its results in the order given, at most one wait, then the sums on the host.
template <typename... Outs>
int deliver(hipStream_t st, Outs &...outs) {
    int rc = SGA_OK;
    ((rc = rc != SGA_OK ? rc : outs.flush(st)), ...);
    if (rc != SGA_OK) return rc;
    if (((outs.copied && outs.host) || ...)) HIPCHK(hipStreamSynchronize(st));
    (outs.land(), ...);
    return SGA_OK;
}

// ---- the problem: what a setter (sga_set_*) computes and allocates.  None of it is the next problem's, whichever setter
// that is and whether or not it assigns the member itself: sga_engine::free_problem() -- every setter -- resets the record.
struct ProblemState {
    int n = 0;
    int n_models = 1;  // dense batches: models stacked row-wise, replicas split evenly
    // sga_set_dense_shared: the n_models models hold ONE coupling matrix (J_packed, J_bits: n rows) and differ in h alone
    // ([n_models][n]; diag and row_nnz are repeated per model, so the kernels index them as they index a stacked batch's)
    // sga_set_csr_shared (csr && shared_j): ONE set of rows (rowptr, cv, diag: n rows) under n_models field vectors, h
    // [n_models][n]; the kernels add model * n to h alone
    bool shared_j = false;
    // ragged CSR batches (sga_set_csr_batch): n_models CSR problems of any sizes concatenated row-wise, replicas split
    // evenly; n = the largest model's spins (the replica layout), n_rows = the rows of the concatenation
    bool ragged = false;
    int n_rows = 0;
    std::vector<int> model_n, model_row0;
    int2 *d_models = nullptr;  // [n_models] {first row, spins}: what the ragged kernels read -- a view inside h's
    int ragged_at = 0;         // allocation, never released; ragged_at floats in: SweepArgs::ragged
    bool csr = false;
    bool want_i8 = false, acc64 = false;
    bool acc_canon = false;  // acc64 and the fp64 row sum is not provably exact: canonical summation order
    bool use_t2 = false;           // ternary J as two bit-planes for the production sweeps
    unsigned int *J_bits = nullptr;  // [2][n][ld/32]
    float *row_nnz = nullptr;        // [n]
    void *J_packed = nullptr;  // [n][ldj] float | int8
    long long ldj = 0;  // row stride of J_packed: n rounded up to 128 bytes
    int32_t *rowptr = nullptr, *colidx = nullptr;  // rowptr: only while the layout has < 2^31 entries
    long long *rowptr64 = nullptr;                  // always (energy / single-site kernels)
    int4 *rowinfo = nullptr;     // slotted layout, per row: first slot, slots, offset of a zero slot, h (wide sweep forms)
    bool slotted = false;        // rows padded to whole 64-entry slots (value-0 entries behind each row)
    bool csr_sorted = false;     // rows strictly sorted by column: no duplicate entries
    uint32_t *cvp = nullptr;     // slotted layout with packed entries (24-bit column | int8 value << 24), on demand
    bool cvp_tried = false;      // packing was attempted for this problem (values may not fit)
    int table_scale = 1;         // CSR accept table: entry q stands for dE = 2 q / table_scale
    long long layout_entries = 0;  // entries of the layout the kernels read (nnz + padding)
    long long max_row_len = 0;     // entries of the longest row
    float *val = nullptr;   // colidx / val: only while the structure is being checked
    int2 *cv = nullptr;     // [nnz] interleaved (column, value bits): what the kernels read
    long long nnz = 0;
    float *h = nullptr, *diag = nullptr;
    // TSP-structured couplings, never stored (sga_set_tsp): scaled distance tables + penalties
    bool tsp = false, tsp_exact = true;
    float *nd4 = nullptr, *nd4t = nullptr;
    sga::TspArgs tsp_args{};
    // couplings as a sum of complete graphs on groups, never stored (sga_set_groups): site -> group table, group -> members
    bool groups = false;
    int *g_gptr = nullptr, *g_members = nullptr;
    int2 *g_gent = nullptr;
    long long *g_member_ptr = nullptr;
    float *g_coeff = nullptr;  // [n_groups] as handed over (checksum)
    int *g_rptr = nullptr;     // the stored remainder of sga_set_groups_csr (null: none): extents [n + 1] ...
    int2 *g_rent = nullptr;    // ... and (column, value bits) entries; counts in group_args.rest
    long long g_memberships = 0;  // entries of the site -> group table
    int g_max_size = 0, g_kmax = 0, g_exp = 0;  // largest group, most memberships of one site, k of the 2^-k grid
    sga::GroupArgs group_args{};
    bool implicit() const { return tsp || groups; }  // structured couplings, none stored
    double *epart = nullptr;  // per-slice energy sums (few replicas)
    size_t epart_bytes = 0;
    std::string tune_table;  // what the last sga_autotune measured: "candidate=ms per sweep;..." (sga_get_autotune_table)
    bool consistent_dE = true;  // J symmetric with zero diagonal: dE of the rule == energy change
    // cached-local-field sweep (sweep_clf_impl.h)
    bool from_dense = false;  // CSR problem built from a sparse matrix handed over dense (sga_set_dense, SGA_J_AUTO)
    bool clf_problem = false;  // dense (one model or a batch, over all stacked rows), J integer valued, h in multiples of 1/2, symmetric, zero diagonal, sums < 2^24
    float row_abs_max = 0.0f;  // max_i(sum_j |J_ij| + |h_i|)
    int j_abs_max = 0;         // ceil(max |J_ij|): the most one flip moves another site's field (several accepts per round: sweep_clfb_impl.h)
    // ... of CSR problems (sweep_clf_csr.hip): integer J, rows strictly sorted, max_i sum_j |J_ij| < 2^15, the accept
    // table applies, dE of the rule == energy change; the fields are then D = J s as int16, h stays outside
    bool clf_csr_problem = false;
    // ... of ragged CSR batches under option "ragged_field_cache": the first model that keeps the batch off the int16
    // form and why (empty: the batch qualifies, or the option is off)
    std::string clf_ragged_why;
    // ... or, with option "clf_fixed_point", as exact fixed point: D = 2^k J s as int32 | int64 (any fp32 J whose row
    // sums are exact, h fp32 beside it): the width (0 = not this form), k, and why the form does not apply (nullptr: it does)
    // -- for dense couplings too (sweep_clf_fx.hip: the dense problems clf_problem does not take)
    int clf_fx_bits = 0, clf_fx_k = 0;
    const char *clf_fx_why = nullptr;
    const char *clf_why = nullptr;  // dense problems the integer form does not take: which condition failed (set-time scan)
    float row_j_abs_max = 0.0f;  // max_i sum_j |J_ij|
    float csr_row_abs_max = 0.0f;  // CSR: max_i (sum_j |J_ij| + |h_i|): no |fk| of a move exceeds it
    int *hq = nullptr;           // [n] table_scale * h_i as integers (built with the first cached sweep)
    int clf_scale = 1, clf_bits = 16;
    long long ldf = 0;  // row stride of ReplicaState::fields
    int csr_acc = sga::CSR_ACC_F64_CANON;  // CSR: how the sweep kernels form a row sum (set time)
    // what the set-time scans wrote, as read back by the setter (sga_get_scan_summary): dense the eight words of
    // classify_dense, CSR the CSR_* words and the longest row per model; empty: none kept (implicit couplings)
    std::vector<int32_t> scan_words;
    int scan_per_model = 0;  // words per model (dense: the one stacked scan)
    bool csr_x_exact = false;  // CSR: the fp64 sum X = sum_i mv_i s_i of an energy is exact in any order (set time)
    // Latched per replica set: sga_init_replicas writes these for the replicas it lays out, and they stay -- through
    // free_replicas(), for sga_describe and sga_get_route_query -- until the next problem.
    long long ld = 0;   // spins per replica (whole chunks)
    int waves = 0, cpw = 0;
    int waves_t2 = 0, cpw_t2 = 0;    // bit-plane geometry (waves/cpw then describe the int8 fallback)
    bool big = false;  // CSR sweeps with bit spins in LDS
    int big_form = 0;  // 0 int8 spins | 1 bits, one replica per workgroup, 64-bit extents | 2 bits, narrow
    int table_m = 0;  // integer problems: largest possible |dE| / 2 (0 = not integer / too big)
    int tsp_waves = 0, tsp_passes = 0;
    int csr_storage_latched = SGA_CSR_STORAGE_AUTO;  // what the current replicas were laid out for (asked: csr_storage)

    void reset(Release release) {
        release_all({J_packed, J_bits, row_nnz, rowptr, rowptr64, rowinfo, cvp, colidx, val, cv, h, diag, nd4, nd4t, hq, g_gptr,
                     g_members, g_gent, g_member_ptr, g_coeff, g_rptr, g_rent, epart},
                    release);
        *this = ProblemState{};
    }
};

// ---- the replicas: what sga_init_replicas, the ladder and the sweeps keep per replica set.  sga_engine::free_replicas()
// -- every setter before free_problem(), sga_init_replicas itself -- resets the record.
struct ReplicaState {
    int R = 0, Rg = 0;
    int8_t *spins = nullptr, *best_spins = nullptr;
    double *energy = nullptr, *best_energy = nullptr, *rep_temp = nullptr;
    unsigned long long *n_acc = nullptr;
    // ladder
    int n_ladders = 0;
    double *slot_temps = nullptr;
    int32_t *slot_to_rep = nullptr;
    long long *ex_attempts = nullptr, *ex_accepts = nullptr;
    float *wolff_u = nullptr;        // recorded uniforms of the Wolff rule [R][wolff_cap] (parity tests)
    long long *wolff_cursor = nullptr;  // [R]
    long long wolff_cap = 0;
    // cached-local-field sweep
    void *fields = nullptr;    // [R][ldf] int16 | int32: clf_scale * (J s + h), valid while fields_valid
    bool fields_valid = false;
    void *ybuf = nullptr;      // [count][ldj] int32 | float: scratch of the all-replica field pass
    size_t ybuf_bytes = 0;
    // The cached-field modes look at the acceptance of the last sweeps now and then (host read-back of the per-replica
    // counters): which replicas run on which kernel family, and in which form of the cached one (sga_route.cpp, look)
    sga_route::ReplicaRouting routing;
    int *d_rep_lists = nullptr;         // [2][R]: the cached-field kernel's replicas, then the row kernels'

    void reset(Release release) {
        release_all({spins, best_spins, energy, best_energy, rep_temp, n_acc, slot_temps, slot_to_rep, ex_attempts, ex_accepts,
                     wolff_u, wolff_cursor, fields, ybuf, d_rep_lists},
                    release);
        *this = ReplicaState{};
    }
};

}  // namespace sga_impl

using namespace sga_impl;

// What no reset touches stays here, grouped by why it survives.
struct sga_engine : ProblemState, ReplicaState {
    // -- the caller's choices: they hold for every later problem (include/sga.h)
    long long opt[OPT_COUNT];  // sga_set_option values (defaults: OPT_DEFS, the environment read once in sga_create)
    // an option latched at sga_set_* (bit 2) / sga_init_replicas (bit 1) changed afterwards: the next sweep says so
    // instead of silently running the form the old value chose
    int opt_stale = 0;
    const char *opt_stale_key = nullptr;
    // The caller's own sga_set_tuning waves and option "csr_updates_per_step".  sga_autotune writes its pick into tune_waves
    // and opt[] for the problem it measured; free_problem() -- every setter -- goes back to these.
    int caller_tune_waves = 0;
    long long caller_csr_ups = -1;
    int tune_waves = 0, tune_spl = 0;
    int csr_storage = SGA_CSR_STORAGE_AUTO;  // sga_set_csr_storage (laid out for: csr_storage_latched)
    int field_cache = SGA_FIELD_CACHE_OFF;   // sga_set_field_cache
    int rule = SGA_RULE_METROPOLIS;          // sga_set_update_rule

    // -- as long as the engine: made in sga_create or on first use, released in sga_destroy
    int device = 0;
    int cus = 256;  // compute units of the device
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t aux_stream = nullptr;   // the second launch of a mixed sweep
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    char last_kernel[512] = {0};        // the instantiation this engine's last sweep launch ran (sga_get_last_kernel)
    int *d_count = nullptr;
    int *d_flags = nullptr;  // [16] value / structure scan results of the set_* calls (one per engine)
    // staging slots: 0 sched, 1 replay sites, 2 replay u, 3 energy trace, 4 accept trace,
    // 5 dE trace, 6 exchange energies, 7 exchange start, 8 exchange u
    Scratch scratch[9];
    Scratch point_sites, point_out;  // single-site operators
    Scratch csr_energy;              // transposed spin bits + partial sums of the all-replica CSR energy pass
    // timing
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    int64_t launches = 0;
    double total_ms = 0.0;

    // -- the window forms (row-shared windows, their tiles, sequential windows): everything they keep between sweeps, ordered
    // by lifetime (sga_windows.h).  It holds the caller's seq_w and the autotuner's suspend beside what its own three resets
    // drop for the next plan, replica set and problem: never assigned wholesale.
    sga_windows::WindowState win;
    void free_row_shared() { win.next_plan(dev_release); }

    // -- the random stream's coordinates and the counters: sga_set_seed and sga_get_sweep_counter work on an engine without
    // replicas, and sga_init_replicas (or an import of state) overwrites what it means to
    int replica0 = 0;
    uint64_t seed = 0;
    int sstride = 0;
    long long attempted = 0;  // per replica
    uint32_t sweeps_done = 0, rounds = 0;

    void free_problem(Release release = dev_release) {
        ProblemState::reset(release);
        win.next_problem(release);
        // sga_autotune's pick ends with the problem it was measured on (include/sga.h)
        tune_waves = caller_tune_waves;
        opt[OPT_CSR_UPDATES_PER_STEP] = caller_csr_ups;
    }
    void free_replicas(Release release = dev_release) {
        ReplicaState::reset(release);
        win.next_replicas(release);
    }
};

namespace sga_impl {

// ragged CSR batches: the model of local replica r and its spins (any other engine: model 0 with n spins)
inline int model_of(const sga_engine *e, int r) {
    return e->ragged && e->Rg > 0 ? (e->replica0 + r) / (e->Rg / e->n_models) : 0;
}
// elements between two models' coupling blocks as the kernels add them (SweepArgs::model_stride_j): 0 = one shared matrix
inline long long model_stride_j(const sga_engine *e) { return e->shared_j ? 0 : (long long)e->n * e->ldj; }
inline int spins_of(const sga_engine *e, int r) { return e->ragged ? e->model_n[(size_t)model_of(e, r)] : e->n; }
// The replica geometry and the random stream's seed into an argument record that carries them (ClusterArgs, ResampleArgs,
// PairOverlapArgs, ClassOverlapArgs, SweepArgs: the members keep their places, a record without seed takes no seed_into).
template <typename Args>
inline void geometry_into(Args &a, const sga_engine *e) {
    a.n = e->n, a.sstride = e->sstride, a.R = e->R, a.replica0 = static_cast<decltype(a.replica0)>(e->replica0);
}
template <typename Args>
inline void seed_into(Args &a, const sga_engine *e) { a.seed_lo = (uint32_t)e->seed, a.seed_hi = (uint32_t)(e->seed >> 32); }

inline int elems_per_chunk(bool i8) { return i8 ? 1024 : 256; }
// Zeroed (column 0, value 0) entries behind the CSR entry array.  The sweep kernels load a row's entries without
// a bounds test and mask what lies past the row's end when summing: the one-update forms reach up to 64 entries
// past the last row's first entry (also the wide forms' zero slot), the several-updates-per-step builds for rows of
// 65 ... 256 entries (sweep_csr_rows.hip: 16 lanes x 8 | 16 entries per lane) up to 256.
constexpr long long CSR_TAIL_PAD = 256;
constexpr int T2_ELEMS_PER_CHUNK = 8192;  // 1 KiB of one bit-plane
inline long long t2_row_bits(int n) { return ((long long)n + 127) / 128 * 128; }  // 16-byte granules

// ---- sga_engine.cpp
sga_route_query route_query_of(const sga_engine *e);  // the engine's own traits / replicas / options as a query
bool fields_pass_applies(const sga_engine *e, int count);
int fields_pass(sga_engine *e, int r0, int count, double *energy, void *fields);
bool clf_possible(const sga_engine *e, const char **why);
bool clf_active(const sga_engine *e);
int ensure_fields(sga_engine *e);
int recompute_energy_range(sga_engine *e, int r0, int count);
int ensure_packed(sga_engine *e);
// ---- sga_windows.cpp: each of the four a line over the pure half (sga_windows.h), asked of window_traits_of(e)
sga_windows::WindowTraits window_traits_of(const sga_engine *e);
// W of the row-shared windows for a sweep whose arguments are the production ones (lean), 0: the row-per-proposal kernel
int row_shared_window(const sga_engine *e, bool lean);
// magnitude planes of the row-shared form that serves the problem (0: none); *grid: 0 the integer form, else 1 + k
int row_shared_form_planes(const sga_engine *e, int *grid);
// the tiles of its fields kernel (option "row_shared_fields"); S = 0: the per-site kernel, *why the reason
sga::RowSharedTiles row_shared_tiles(const sga_engine *e, const char **why);
// the replica groups of a row-shared sweep of window rs_w over `tiles` (sga_set_replica_groups, or the rule's count); one
// wherever the form admits none, *why the reason where more were asked for
int replica_groups(const sga_engine *e, int rs_w, const sga::RowSharedTiles &tiles, bool energy_trace, const char **why);
// the sequential windows (sga_set_sequential_windows) as a sequential, untraced sweep of this engine would run them:
// W = 0 where the row-per-proposal kernel runs (base is left null: the scratch is the sweep's)
sga::SeqWindows sequential_windows(const sga_engine *e);
// The window forms of one sga_sweep call off the cached fields and the exact mode: rs_w, rs_tiles and seq as the launches
// take them.  In this order: the row-shared scratch (and, once per problem, the planes), the tile kernel's LDS request,
// the sequential scratch and int8 copy.  Every failure leaves the row-per-proposal kernel; a refused LDS request and a
// failed int8 copy are remembered for the problem.
// rs_groups: the replica groups the row-shared launch runs (their streams and events made here, once per engine).
void plan_windows(sga_engine *e, bool lean_call, bool sequential_call, bool energy_trace, int &rs_w, sga::RowSharedTiles &rs_tiles,
                  int &rs_groups, sga::SeqWindows &seq);
// ---- sga_problem.cpp
bool csr_rows_medium(const sga_engine *e);
int csr_updates_per_step(const sga_engine *e);
int ensure_slotted(sga_engine *e);
int ensure_packed_entries(sga_engine *e);

}  // namespace sga_impl

#endif  // SGA_ENGINE_IMPL_H
