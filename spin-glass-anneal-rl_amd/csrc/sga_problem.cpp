// sga_problem.cpp -- the problem side of the C ABI (include/sga.h): sga_set_dense / sga_set_dense_batch, sga_set_csr /
// sga_set_csr64, sga_set_tsp.  Value and structure scans on the device, the packed layouts the kernels read, CSR row
// layouts (plain / 64-entry slots / packed entries).  Which arithmetic a problem admits: sga_classify.cpp; which form it
// then runs in: sga_route.cpp.
#include "sga_classify.h"
#include "sga_engine_impl.h"

namespace {

static_assert(sga_classify::ACC_F32_TABLE == sga::CSR_ACC_F32_TABLE && sga_classify::ACC_F32 == sga::CSR_ACC_F32 &&
              sga_classify::ACC_F64 == sga::CSR_ACC_F64 && sga_classify::ACC_F64_CANON == sga::CSR_ACC_F64_CANON, "acc classes");

// the CSR scans' flag words as sga_classify reads them
sga_classify::CsrScan csr_scan_of(const int *flags) {
    sga_classify::CsrScan s;
    s.not_integral = flags[sga::CSR_NOT_INTEGRAL];
    s.unsorted = flags[sga::CSR_UNSORTED] != 0;
    s.diagonal = flags[sga::CSR_DIAGONAL] != 0;
    s.asymmetric = flags[sga::CSR_ASYMMETRIC] != 0;
    std::memcpy(&s.row_abs_max, &flags[sga::CSR_ROW_ABS_MAX], sizeof(float));
    std::memcpy(&s.row_j_abs_max, &flags[sga::CSR_ROW_J_ABS_MAX], sizeof(float));
    s.exp_hi_word = flags[sga::CSR_EXP_HI];
    s.exp_lo_word = flags[sga::CSR_EXP_LO];
    return s;
}

// a model's CSR words as sga_get_scan_summary hands them out: the CSR_* words in enum order, then the longest row
void keep_csr_scan(sga_engine *e, const int *flags, long long longest_row) {
    e->scan_per_model = sga::CSR_FLAG_COUNT + 1;
    e->scan_words.insert(e->scan_words.end(), flags, flags + sga::CSR_FLAG_COUNT);
    e->scan_words.push_back((int32_t)std::min<long long>(longest_row, INT32_MAX));
}

const char *const NON_FINITE_MSG = "non-finite value (NaN or +-Inf) in J or h";

// Pack the caller's fp32 matrix (device pointer `src`, row stride ld_src) into the engine's
// layout(s): rows packed to 128 bytes, not padded to the kernel's whole chunks (2.4 % fewer bytes
// per attempt at n = 10^4); lanes past a row's end re-read its first granule.
int pack_dense(sga_engine *e, const float *src, long long ld_src) {
    const long long rows = e->shared_j ? e->n : (long long)e->n_models * e->n;  // (one shared matrix: its n rows)
    const long long elem = e->want_i8 ? 1 : 4;
    const long long ldj = ((long long)e->n * elem + 127) / 128 * 128 / elem;
    const size_t bytes = (size_t)rows * ldj * elem;
    HIPCHK(hipMalloc(&e->J_packed, bytes));
    HIPCHK(sga::launch_repack_dense(src, ld_src, rows, e->n, e->J_packed, ldj, e->want_i8, e->diag,
                                    e->stream));
    e->ldj = ldj;
    if (e->use_t2) {
        // a plane's rows are packed at 16-byte granularity, not padded to the kernel's 1-KiB chunks
        // (n = 10^4: 1264 B instead of 2048 B per row and plane -- this form is bound by the bytes
        // it pulls through the cache hierarchy); the kernel masks the lanes past a row's end
        const long long row_bits = t2_row_bits(e->n);
        HIPCHK(hipMalloc(&e->J_bits, sizeof(unsigned int) * 2 * (size_t)e->n * (size_t)(row_bits / 32)));
        // (row_nnz is read as diag is, at model * n: a shared matrix repeats it per model)
        HIPCHK(hipMalloc(&e->row_nnz, sizeof(float) * (size_t)e->n * (size_t)(e->shared_j ? e->n_models : 1)));
        HIPCHK(sga::launch_repack_tern2(src, ld_src, e->n, e->J_bits, row_bits, e->row_nnz, e->stream));
    }
    // one shared matrix: diag (and row_nnz) once more per model -- the kernels index them as a stacked batch's, no
    // branch in their loops
    for (int m = 1; e->shared_j && m < e->n_models; ++m) {
        HIPCHK(hipMemcpyAsync(e->diag + (size_t)m * e->n, e->diag, sizeof(float) * (size_t)e->n, hipMemcpyDeviceToDevice, e->stream));
        if (e->row_nnz)
            HIPCHK(hipMemcpyAsync(e->row_nnz + (size_t)m * e->n, e->row_nnz, sizeof(float) * (size_t)e->n,
                                  hipMemcpyDeviceToDevice, e->stream));
    }
    return SGA_OK;
}

// Row extents of the layout the kernels read: dst[i] = prefix sum of the rows' lengths, each rounded
// up to whole 64-entry slots when `slotted`.  n <= ~1.3e6 rows: done on the host at set time.
//
// Slotted layouts also get the wide forms' per-row record (rowinfo: first slot, slot count | entries in
// the last slot << 24, slots from the first slot to an all-zero slot, h): a wave asks for a fixed number of slots per row and
// the ones past the row's end read that zero slot (value 0: nothing to mask when the row is
// summed).  The zero slot is the 64 zeroed entries behind the array; layouts beyond 2^21 slots
// (1 GB) get one more inside after every 2^21 slots -- it rides at the end of the row before it,
// like slot padding -- so that the offset always fits the 32-bit lane offset of a load.
int build_layout(sga_engine *e, const std::vector<long long> &src, bool slotted) {
    const int n = e->n;
    long long ZERO_SLOT_EVERY = 1ll << 21;
    if (e->opt[OPT_ZERO_SLOT_EVERY] > 0)  // parity tests: zero slots inside small layouts
        ZERO_SLOT_EVERY = std::max(1ll, std::min(ZERO_SLOT_EVERY, e->opt[OPT_ZERO_SLOT_EVERY]));
    std::vector<long long> dst((size_t)n + 1);
    std::vector<int4> info(slotted ? (size_t)n : 0);
    std::vector<int32_t> narrow;
    std::vector<std::pair<int, long long>> zero_after;  // (row, slot number) of the zero slots inside
    long long at = 0, since = 0;
    for (int i = 0; i < n; ++i) {
        dst[(size_t)i] = at;
        const long long len = src[(size_t)i + 1] - src[(size_t)i];
        // (src may be a padded layout being re-padded: slot padding never adds a slot)
        e->max_row_len = i == 0 ? len : std::max(e->max_row_len, len);
        if (!slotted) {
            at += len;
            continue;
        }
        const long long slots = (len + 63) / 64;
        // .y: slot count | entries in the last slot << 24 (lanes beyond them read the zero slot: no HBM
        // traffic for the padding's cache lines)
        if (slots >= (1 << 24)) return fail(SGA_ERR_UNSUPPORTED, "CSR row too long for the slot addressing");
        info[(size_t)i] = make_int4((int)(at >> 6), (int)(slots | ((len - 64 * (slots - 1)) << 24)), 0, 0);
        if (slots == 0) info[(size_t)i].y = 0;
        at += slots * 64;
        since += slots;
        if (since >= ZERO_SLOT_EVERY && i + 1 < n) {
            zero_after.emplace_back(i, at >> 6);
            at += 64;
            since = 0;
        }
    }
    dst[(size_t)n] = at;
    if (slotted) {
        if ((at >> 6) >= (long long)INT32_MAX) return fail(SGA_ERR_UNSUPPORTED, "CSR problem too large");
        zero_after.emplace_back(n - 1, at >> 6);  // the zeroed entries behind the array
        size_t z = 0;
        for (int i = 0; i < n; ++i) {
            while (zero_after[z].first < i) ++z;
            info[(size_t)i].z = (int)(zero_after[z].second - info[(size_t)i].x);
            if (info[(size_t)i].z >= (1 << 23)) return fail(SGA_ERR_UNSUPPORTED, "CSR row too long for the slot addressing");
        }
    }
    dev_free(e->rowptr);
    dev_free(e->rowinfo);
    const size_t np1 = (size_t)n + 1;
    HIPCHK(hipMemcpyAsync(e->rowptr64, dst.data(), sizeof(long long) * np1, hipMemcpyHostToDevice, e->stream));
    if (at < (long long)INT32_MAX) {
        narrow.assign(dst.begin(), dst.end());
        HIPCHK(hipMalloc(&e->rowptr, sizeof(int32_t) * np1));
        HIPCHK(hipMemcpyAsync(e->rowptr, narrow.data(), sizeof(int32_t) * np1, hipMemcpyHostToDevice, e->stream));
    }
    if (slotted) {
        HIPCHK(hipMalloc(&e->rowinfo, sizeof(int4) * (size_t)n));
        HIPCHK(hipMemcpyAsync(e->rowinfo, info.data(), sizeof(int4) * (size_t)n, hipMemcpyHostToDevice, e->stream));
        HIPCHK(sga::launch_rowinfo_fields(e->rowinfo, e->h, n, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));  // the host vectors go out of scope
    e->slotted = slotted;
    e->layout_entries = at;
    return SGA_OK;
}

}  // namespace

namespace sga_impl {

// several updates per step (sweep_csr_rows.hip): which problems, how many -- sga_route.cpp
bool csr_rows_medium(const sga_engine *e) { return sga_route::csr_rows_medium(route_query_of(e)); }
int csr_updates_per_step(const sga_engine *e) { return sga_route::csr_updates_per_step(route_query_of(e)); }

// The wide sweep forms (a row dealt to several waves) address rows by 64-entry slots: re-pad an
// unpadded layout on demand (short-row problems run wide only when tuning asks for it).
int ensure_slotted(sga_engine *e) {
    if (!e->csr || e->slotted) return SGA_OK;
    const size_t np1 = (size_t)e->n + 1;
    std::vector<long long> src(np1);
    HIPCHK(hipMemcpy(src.data(), e->rowptr64, sizeof(long long) * np1, hipMemcpyDeviceToHost));
    long long *old_ptr = nullptr;
    HIPCHK(hipMalloc(&old_ptr, sizeof(long long) * np1));
    hipError_t he = hipMemcpy(old_ptr, e->rowptr64, sizeof(long long) * np1, hipMemcpyDeviceToDevice);
    int2 *old_cv = e->cv;
    int rc = he == hipSuccess ? build_layout(e, src, true) : fail(SGA_ERR_DEVICE, hipGetErrorString(he));
    if (rc == SGA_OK) {
        e->cv = nullptr;
        he = hipMalloc(&e->cv, sizeof(int2) * (size_t)(e->layout_entries + CSR_TAIL_PAD));
        if (he == hipSuccess) he = hipMemsetAsync(e->cv + e->layout_entries, 0, sizeof(int2) * CSR_TAIL_PAD, e->stream);
        if (he == hipSuccess)
            he = sga::launch_pack_cv_rows(old_ptr, e->rowptr64, nullptr, nullptr, old_cv, e->cv, e->n, e->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
        if (he != hipSuccess) rc = fail(he == hipErrorOutOfMemory ? SGA_ERR_MEMORY : SGA_ERR_DEVICE, hipGetErrorString(he));
        dev_free(old_cv);
    }
    dev_free(old_ptr);
    if (rc != SGA_OK) {
        // build_layout may already have overwritten the extents while the entries are still the old
        // ones (or gone): no half-converted layout survives -- the engine is back to "no couplings set"
        const std::string msg = g_last_error;
        (void)hipStreamSynchronize(e->stream);
        e->free_replicas();
        e->free_problem();
        return fail(rc, msg + " (re-padding the CSR layout failed: set the couplings again)");
    }
    return rc;
}

// Packed entries for the bit-spin wide forms of integer-valued problems (|J| <= 127, n < 2^24): one
// dword per entry, the same slots (256 bytes each) -- half the bytes of a row.  Built on demand from the
// slotted layout; the (column, value) layout stays (energy kernels, traced sweeps).
int ensure_packed_entries(sga_engine *e) {
    if (e->cvp || e->cvp_tried) return SGA_OK;
    e->cvp_tried = true;
    if (!e->csr || !e->slotted || e->n >= (1 << 24) ||
        (e->csr_acc != sga::CSR_ACC_F32 && e->csr_acc != sga::CSR_ACC_F32_TABLE))
        return SGA_OK;
    const size_t count = (size_t)e->layout_entries + 64;  // the zero slot behind the array included
    hipError_t he = hipMalloc(&e->cvp, sizeof(uint32_t) * count);
    if (he != hipSuccess) {
        e->cvp = nullptr;
        (void)hipGetLastError();
        return SGA_OK;  // no room: the unpacked layout serves
    }
    int bad = 0;
    he = hipMemsetAsync(e->d_flags, 0, sizeof(int), e->stream);
    if (he == hipSuccess) he = sga::launch_pack_entries(e->cv, e->cvp, (long long)count, e->d_flags, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(&bad, e->d_flags, sizeof(int), hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (he != hipSuccess || bad) dev_free(e->cvp);
    if (he != hipSuccess) return fail(SGA_ERR_DEVICE, hipGetErrorString(he));
    return SGA_OK;
}

}  // namespace sga_impl

namespace {

// CSR problem from 32- or 64-bit row extents (host or device pointers).  The structure is
// checked on the device -- a bad extent or column would fault in the sweep kernels -- and the
// same pass classifies the problem: integer valued (accept table, fp32-exact row sums),
// symmetric with zero diagonal (dE of the rule == energy change).  Device arrays are read where
// they lie, host arrays are staged; only the interleaved layout stays resident.
//
// n_models > 1 (sga_set_csr_shared): h is [n_models][n], ONE set of rows under n_models field vectors.  The structure is
// checked, classified and packed once, exactly as for one model; the h-dependent scan words ([2], [6]) and with them the
// accept table are taken over all of h -- an exact sum stays exact in a wider class, and a table entry stands for the
// same dE at any scale.
int set_csr_common(sga_engine *e, const void *rowptr, bool wide_extents, const int32_t *colidx,
                          const float *val, const float *h, int n, int64_t nnz, int n_models = 1) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (!rowptr || !h || n <= 0 || nnz < 0 || (nnz > 0 && (!colidx || !val)) || n_models <= 0)
        return fail(SGA_ERR_INVALID, "bad CSR problem arguments");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->free_replicas();
    e->free_problem();
    e->opt_stale = 0;
    e->csr = true;
    e->from_dense = false;
    e->n = n;
    e->n_models = n_models;
    e->shared_j = n_models > 1;  // (one model: sga_set_csr in every respect)
    e->nnz = nnz;
    const size_t np1 = (size_t)n + 1;
    if (!wide_extents && nnz >= (int64_t)INT32_MAX) {
        e->free_problem();
        return fail(SGA_ERR_INVALID, "nnz >= 2^31 needs 64-bit row extents (sga_set_csr64)");
    }
    HIPCHK(hipMalloc(&e->rowptr64, sizeof(long long) * np1));
    if (wide_extents) {
        HIPCHK(hipMemcpyAsync(e->rowptr64, rowptr, sizeof(long long) * np1, hipMemcpyDefault, e->stream));
    } else {
        HIPCHK(e->scratch[1].reserve(sizeof(int32_t) * np1));
        int32_t *tmp = static_cast<int32_t *>(e->scratch[1].ptr);
        HIPCHK(hipMemcpyAsync(tmp, rowptr, sizeof(int32_t) * np1, hipMemcpyDefault, e->stream));
        HIPCHK(sga::launch_widen_rowptr(tmp, e->rowptr64, (long long)np1, e->stream));
    }
    const size_t nz = (size_t)std::max<int64_t>(nnz, 1);
    // the caller's arrays: borrowed when they are device memory, staged otherwise (freed below)
    const int32_t *ci = colidx;
    const float *vv = val;
    if (nnz > 0 && !is_device_ptr(colidx)) {
        HIPCHK(hipMalloc(&e->colidx, sizeof(int32_t) * nz));
        HIPCHK(hipMemcpyAsync(e->colidx, colidx, sizeof(int32_t) * nz, hipMemcpyHostToDevice, e->stream));
        ci = e->colidx;
    }
    if (nnz > 0 && !is_device_ptr(val)) {
        HIPCHK(hipMalloc(&e->val, sizeof(float) * nz));
        HIPCHK(hipMemcpyAsync(e->val, val, sizeof(float) * nz, hipMemcpyHostToDevice, e->stream));
        vv = e->val;
    }
    HIPCHK(hipMalloc(&e->h, sizeof(float) * (size_t)n * (size_t)n_models));
    HIPCHK(hipMemcpyAsync(e->h, h, sizeof(float) * (size_t)n * (size_t)n_models, hipMemcpyDefault, e->stream));
    HIPCHK(hipMalloc(&e->diag, sizeof(float) * (size_t)n));  // (J's: once, whatever n_models)

    int *d_flags = e->d_flags;
    int flags[sga::CSR_FLAG_COUNT] = {0};
    static_assert(sga::CSR_FLAG_COUNT <= 16, "engine flag words");
    auto read_flags = [&]() -> hipError_t {
        hipError_t he = hipMemcpyAsync(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, e->stream);
        return he == hipSuccess ? hipStreamSynchronize(e->stream) : he;
    };
    auto bail = [&](int code, const char *msg) {
        e->free_problem();
        return fail(code, msg);
    };
    hipError_t he = hipMemsetAsync(d_flags, 0, sizeof(flags), e->stream);
    if (he == hipSuccess) he = sga::launch_csr_check_rowptr(e->rowptr64, n, nnz, d_flags, e->stream);
    if (he == hipSuccess) he = read_flags();
    if (he != hipSuccess) return bail(SGA_ERR_DEVICE, hipGetErrorString(he));
    if (flags[sga::CSR_BAD_ROWPTR])
        return bail(SGA_ERR_INVALID, "CSR rowptr is not monotone or does not span [0, nnz]");
    he = sga::launch_csr_scan(e->rowptr64, ci, vv, e->h, n, d_flags, e->stream, n_models);
    if (he == hipSuccess) he = read_flags();
    if (he != hipSuccess) return bail(SGA_ERR_DEVICE, hipGetErrorString(he));
    if (flags[sga::CSR_BAD_COLUMN]) return bail(SGA_ERR_INVALID, "CSR column index out of range");
    if (flags[sga::CSR_NOT_INTEGRAL] & sga::SCAN_NON_FINITE) return bail(SGA_ERR_INVALID, NON_FINITE_MSG);
    // symmetric with zero diagonal?  Sorted rows: one binary search per entry; unsorted rows are
    // compared by linear scans while that stays cheap, else treated as asymmetric (exact-energy
    // mode: slower, never wrong)
    const bool sorted = !flags[sga::CSR_UNSORTED];
    e->csr_sorted = sorted;
    const double avg_deg = (double)nnz / n;
    if (sorted || (double)nnz * avg_deg <= 4.0e10) {
        he = sga::launch_csr_symmetry(e->rowptr64, ci, vv, n, sorted, d_flags, e->stream);
        if (he == hipSuccess) he = read_flags();
        if (he != hipSuccess) return bail(SGA_ERR_DEVICE, hipGetErrorString(he));
    } else {
        flags[sga::CSR_ASYMMETRIC] = 1;
    }
    HIPCHK(sga::launch_gather_diag_csr(e->rowptr64, ci, vv, n, e->diag, e->stream));
    std::vector<long long> src(np1);
    HIPCHK(hipMemcpyAsync(src.data(), e->rowptr64, sizeof(long long) * np1, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    {
        // the class of the problem (sga_classify.cpp), once the longest row is known
        long long max_len = 0;
        for (int i = 0; i < n; ++i) max_len = std::max(max_len, src[(size_t)i + 1] - src[(size_t)i]);
        const sga_classify::CsrClass c = sga_classify::classify_csr(
            csr_scan_of(flags), max_len, n, {e->opt[OPT_HALF_TABLE] != 0, (int)e->opt[OPT_FORCE_CSR_ACC]});
        keep_csr_scan(e, flags, max_len);
        e->consistent_dE = c.consistent_dE;
        e->table_m = c.table_m;
        e->table_scale = c.table_scale;
        e->csr_row_abs_max = c.row_abs_max;
        e->row_j_abs_max = c.row_j_abs_max;
        e->clf_csr_problem = c.clf_int16;
        e->csr_acc = c.acc;
        e->csr_x_exact = c.x_exact;
        if (e->opt[OPT_CLF_FIXED_POINT] == 1 && !e->clf_csr_problem) {  // the problems the int16 form does not take
            const sga_classify::FxVerdict v = sga_classify::csr_fixed_point(c, n);
            e->clf_fx_why = v.why;
            e->clf_fx_bits = v.bits;
            e->clf_fx_k = v.k;
            e->clf_csr_problem = !v.why;
        }
    }
    // The layout the kernels read: (column, value) interleaved, one 8-byte load per entry.  Long
    // rows (mean degree >= 192: the problems that run the wide forms) are padded to whole 64-entry
    // slots; CSR_TAIL_PAD zeroed entries behind the array (an empty last row's slot 0; unmasked row loads).
    long long *src_ptr = nullptr;  // the caller's extents, on the device, while rows are packed
    HIPCHK(hipMalloc(&src_ptr, sizeof(long long) * np1));
    he = hipMemcpyAsync(src_ptr, e->rowptr64, sizeof(long long) * np1, hipMemcpyDeviceToDevice, e->stream);
    int rc = he == hipSuccess ? build_layout(e, src, sga_route::csr_slots_at_set(nnz, n, e->opt[OPT_CSR_SLOTS]))
                              : fail(SGA_ERR_DEVICE, hipGetErrorString(he));
    if (rc == SGA_OK) {
        he = hipMalloc(&e->cv, sizeof(int2) * (size_t)(e->layout_entries + CSR_TAIL_PAD));
        if (he == hipSuccess) he = hipMemsetAsync(e->cv + e->layout_entries, 0, sizeof(int2) * CSR_TAIL_PAD, e->stream);
        if (he == hipSuccess) he = sga::launch_pack_cv_rows(src_ptr, e->rowptr64, ci, vv, nullptr, e->cv, n, e->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
        if (he != hipSuccess) rc = fail(he == hipErrorOutOfMemory ? SGA_ERR_MEMORY : SGA_ERR_DEVICE, hipGetErrorString(he));
    }
    dev_free(src_ptr);
    dev_free(e->colidx);  // staging copies of host arrays (null when the caller's were device memory)
    dev_free(e->val);
    // one wave per replica reads 32-bit extents: a layout beyond them is sga_set_csr64's, which has no shared variant
    if (rc == SGA_OK && e->shared_j && !e->rowptr)
        rc = fail(SGA_ERR_UNSUPPORTED, "shared-coupling CSR batches run one wave per replica (32-bit row extents): this "
                                       "layout needs 64-bit extents");
    if (rc != SGA_OK) e->free_problem();
    return rc;
}

// sga_set_csr_shared: what the caller can get wrong -- extents, columns, non-finite values -- is looked at BEFORE the
// engine lets go of the problem it holds, on staged copies that live for this call only (the two structure scans once
// more, at set time; nothing of the engine but its flag words is written).  Past that point it is set_csr_common.
int set_csr_shared(sga_engine *e, const int32_t *rowptr, const int32_t *colidx, const float *val, const float *H, int n,
                   int64_t nnz, int n_models) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (!rowptr || !H || n <= 0 || nnz < 0 || (nnz > 0 && (!colidx || !val)) || n_models <= 0)
        return fail(SGA_ERR_INVALID, "bad CSR problem arguments");
    if (nnz >= (int64_t)INT32_MAX)
        return fail(SGA_ERR_UNSUPPORTED, "shared-coupling CSR batches take 32-bit row extents (nnz < 2^31)");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    struct Staged {
        int32_t *rp = nullptr, *ci = nullptr;
        long long *rp64 = nullptr;
        float *v = nullptr, *h = nullptr;
        ~Staged() { dev_free(rp), dev_free(ci), dev_free(rp64), dev_free(v), dev_free(h); }
    } t;
    const size_t np1 = (size_t)n + 1, nz = (size_t)std::max<int64_t>(nnz, 1), nh = (size_t)n * (size_t)n_models;
    HIPCHK(hipMalloc(&t.rp, sizeof(int32_t) * np1));
    HIPCHK(hipMalloc(&t.rp64, sizeof(long long) * np1));
    HIPCHK(hipMemcpyAsync(t.rp, rowptr, sizeof(int32_t) * np1, hipMemcpyDefault, e->stream));
    HIPCHK(sga::launch_widen_rowptr(t.rp, t.rp64, (long long)np1, e->stream));
    const int32_t *ci = colidx;
    const float *vv = val, *hh = H;
    if (nnz > 0 && !is_device_ptr(colidx)) {
        HIPCHK(hipMalloc(&t.ci, sizeof(int32_t) * nz));
        HIPCHK(hipMemcpyAsync(t.ci, colidx, sizeof(int32_t) * nz, hipMemcpyHostToDevice, e->stream));
        ci = t.ci;
    }
    if (nnz > 0 && !is_device_ptr(val)) {
        HIPCHK(hipMalloc(&t.v, sizeof(float) * nz));
        HIPCHK(hipMemcpyAsync(t.v, val, sizeof(float) * nz, hipMemcpyHostToDevice, e->stream));
        vv = t.v;
    }
    if (!is_device_ptr(H)) {
        HIPCHK(hipMalloc(&t.h, sizeof(float) * nh));
        HIPCHK(hipMemcpyAsync(t.h, H, sizeof(float) * nh, hipMemcpyHostToDevice, e->stream));
        hh = t.h;
    }
    int flags[sga::CSR_FLAG_COUNT] = {0};
    HIPCHK(hipMemsetAsync(e->d_flags, 0, sizeof(flags), e->stream));
    HIPCHK(sga::launch_csr_check_rowptr(t.rp64, n, nnz, e->d_flags, e->stream));
    HIPCHK(hipMemcpyAsync(flags, e->d_flags, sizeof(flags), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (flags[sga::CSR_BAD_ROWPTR]) return fail(SGA_ERR_INVALID, "CSR rowptr is not monotone or does not span [0, nnz]");
    HIPCHK(sga::launch_csr_scan(t.rp64, ci, vv, hh, n, e->d_flags, e->stream, n_models));
    HIPCHK(hipMemcpyAsync(flags, e->d_flags, sizeof(flags), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (flags[sga::CSR_BAD_COLUMN]) return fail(SGA_ERR_INVALID, "CSR column index out of range");
    if (flags[sga::CSR_NOT_INTEGRAL] & sga::SCAN_NON_FINITE) return fail(SGA_ERR_INVALID, NON_FINITE_MSG);
    // (the staged copies are device memory: set_csr_common borrows them instead of staging again)
    return set_csr_common(e, t.rp, false, ci, vv, hh, n, nnz, n_models);
}

// does the diagonal pack_dense extracted hold a non-zero?  (*out: 0 | 1)
int diag_nonzero(sga_engine *e, long long rows, int *out) {
    std::vector<float> dg((size_t)rows);
    HIPCHK(hipMemcpyAsync(dg.data(), e->diag, sizeof(float) * (size_t)rows, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    *out = 0;
    for (float v : dg) *out = *out || v != 0.0f;
    return SGA_OK;
}

// Sparse couplings handed over as a dense matrix (the reference's IsingModel is dense by default; its assignment
// and scheduling encoders fill 1-2 % of it): with SGA_J_AUTO, one model, n >= 4096, integer-valued J and no row of
// more than 256 non-zeros the problem is taken as CSR -- a proposal then reads its row's entries instead of n
// couplings, and the several-updates-per-step forms apply (sweep_csr_rows.hip).  Integer row sums are exact in
// either form, so the chain is the dense forms' bit for bit.  When: see the call (the cached-field sweep is a dense
// form); never with option "sparse_route" = 0 (A/B switch).
// Returns SGA_OK with *taken = true when the problem was set as CSR.
int route_sparse_dense(sga_engine *e, const float *src, long long ld_src, const float *h, int n, bool *taken) {
    *taken = false;
    int *nnz_d = nullptr;
    HIPCHK(hipMalloc(&nnz_d, sizeof(int) * ((size_t)n + 1)));
    struct Guard {
        int *a = nullptr, *b = nullptr, *c = nullptr;
        float *v = nullptr;
        ~Guard() { dev_free(a), dev_free(b), dev_free(c), dev_free(v); }
    } g;
    g.a = nnz_d;
    HIPCHK(sga::launch_dense_row_nnz(src, ld_src, n, nnz_d, e->stream));
    std::vector<int> len((size_t)n), rp((size_t)n + 1);
    HIPCHK(hipMemcpyAsync(len.data(), nnz_d, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    long long total = 0;
    int longest = 0;
    for (int i = 0; i < n; ++i) {
        rp[(size_t)i] = (int)total;
        total += len[(size_t)i];
        longest = std::max(longest, len[(size_t)i]);
    }
    rp[(size_t)n] = (int)total;
    if (!sga_route::sparse_route_taken(longest, total)) return SGA_OK;
    HIPCHK(hipMalloc(&g.b, sizeof(int) * ((size_t)n + 1)));
    HIPCHK(hipMalloc(&g.c, sizeof(int) * (size_t)total));
    HIPCHK(hipMalloc(&g.v, sizeof(float) * (size_t)total));
    HIPCHK(hipMemcpyAsync(g.b, rp.data(), sizeof(int) * ((size_t)n + 1), hipMemcpyHostToDevice, e->stream));
    HIPCHK(sga::launch_dense_to_csr(src, ld_src, n, g.b, g.c, g.v, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    // (set_csr_common starts from free_problem()'s defaults; what sga_set_dense's scan found stays with the problem)
    const bool want_i8 = e->want_i8, acc64 = e->acc64, acc_canon = e->acc_canon;
    const float row_abs_max = e->row_abs_max;
    const int j_abs_max = e->j_abs_max, clf_scale = e->clf_scale, clf_bits = e->clf_bits;
    const int rc = set_csr_common(e, g.b, false, g.c, g.v, h, n, total);
    if (rc == SGA_OK) {
        *taken = true;
        e->from_dense = true;
        e->want_i8 = want_i8, e->acc64 = acc64, e->acc_canon = acc_canon;
        e->row_abs_max = row_abs_max;
        e->j_abs_max = j_abs_max, e->clf_scale = clf_scale, e->clf_bits = clf_bits;
    }
    return rc;
}

// sga_set_dense / sga_set_dense_batch (J: n_models matrices stacked row-wise) / sga_set_dense_shared (shared: J is ONE
// matrix of n rows, h still [n_models][n]).  A shared problem is scanned, classified and held as the stack of n_models
// copies of J would be -- the same eight scan words, the same batch-wide verdicts -- except that J is read, packed and
// kept once, and that what needs the ROWS to be one matrix (bit-planes; row-shared windows and the matrix-core pass,
// sga_engine.cpp) is open to it.
int set_dense_common(sga_engine *e, const float *J, int64_t ldJ, const float *h, int n, int n_models, int storage,
                     bool shared) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (!J || !h || n <= 0 || ldJ < n || n_models <= 0)
        return fail(SGA_ERR_INVALID, "bad dense problem arguments");
    if (storage < SGA_J_AUTO || storage > SGA_J_T2)
        return fail(SGA_ERR_INVALID, "bad storage selector");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->free_replicas();
    e->free_problem();
    e->opt_stale = 0;
    e->csr = false;
    e->from_dense = false;
    e->table_m = 0;
    e->n = n;
    e->n_models = n_models;
    e->shared_j = shared && n_models > 1;  // (one model: sga_set_dense in every respect)
    const long long rows = (long long)n_models * n;            // rows of h and diag
    const long long j_rows = e->shared_j ? (long long)n : rows;  // rows of J
    // A device matrix is scanned and packed where it lies; a host matrix is staged first.  Either
    // way nothing but the packed layout(s) stays resident (400 MB, not 800, at n = 10^4 fp32).
    const float *src = J;
    long long ld_src = ldJ;
    struct Staged {
        float *p = nullptr;
        ~Staged() { dev_free(p); }
    } staged;
    if (!is_device_ptr(J)) {
        HIPCHK(hipMalloc(&staged.p, sizeof(float) * (size_t)j_rows * n));
        HIPCHK(hipMemcpy2DAsync(staged.p, sizeof(float) * (size_t)n, J, sizeof(float) * (size_t)ldJ,
                                sizeof(float) * (size_t)n, (size_t)j_rows, hipMemcpyHostToDevice, e->stream));
        src = staged.p;
        ld_src = n;
    }
    HIPCHK(hipMalloc(&e->h, sizeof(float) * (size_t)rows));
    HIPCHK(hipMemcpyAsync(e->h, h, sizeof(float) * (size_t)rows, hipMemcpyDefault, e->stream));
    HIPCHK(hipMalloc(&e->diag, sizeof(float) * (size_t)rows));
    // value scans over all models: can J live in int8; is fp32 accumulation exact; is the
    // problem integer valued with few possible uphill moves (per-sweep accept table); is J
    // symmetric with a zero diagonal (dE of the rule == energy change)?
    int *flags = e->d_flags;  // [0..3] value scans, [4] symmetry / diagonal
    unsigned int *uflags = reinterpret_cast<unsigned int *>(flags) + 2;
    int hflags[8] = {1, 1, 0, 1, 1, 0, 0, 0};  // ([7]: max |J_ij| as float bits, launch_dense_row_abs_max)
    HIPCHK(hipMemsetAsync(flags, 0, 8 * sizeof(int), e->stream));
    // (a shared matrix: the J words from one pass over its n rows, the h-dependent ones over all n_models * n fields)
    HIPCHK(sga::launch_scan_values(src, j_rows, n, ld_src, flags, e->stream));
    HIPCHK(sga::launch_dense_row_abs_max(src, ld_src, e->h, j_rows, n, uflags, e->stream, e->shared_j ? n_models : 1));
    HIPCHK(sga::launch_check_symmetric(src, ld_src, j_rows, n, flags + 4, e->stream));
    HIPCHK(hipMemcpyAsync(hflags, flags, sizeof(hflags), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (hflags[3] & sga::SCAN_NON_FINITE) {
        e->free_problem();
        return fail(SGA_ERR_INVALID, NON_FINITE_MSG);
    }
    e->scan_words.assign(hflags, hflags + 8);
    e->scan_per_model = 8;
    // (storage is a matter of the matrices held: a shared problem holds one)
    const sga_classify::DenseClass c =
        sga_classify::classify_dense(hflags, n, e->shared_j ? 1 : n_models, storage, e->opt[OPT_FORCE_DENSE_CANON] != 0);
    e->consistent_dE = c.consistent_dE;
    if ((storage == SGA_J_I8 && !c.fits_i8) || (storage == SGA_J_T2 && !c.ternary)) {
        e->free_problem();  // (no half-set problem: n, h and the scan words are this call's already)
        return fail(SGA_ERR_INVALID, storage == SGA_J_I8 ? "int8 storage requested but J is not integer in [-127,127]"
                                                         : "bit-plane storage needs one model with J in {-1, 0, +1}");
    }
    e->use_t2 = c.use_t2;
    e->want_i8 = c.want_i8;
    e->acc64 = c.acc64;
    e->acc_canon = c.acc_canon;
    e->table_m = c.table_m;
    e->row_abs_max = c.row_abs_max;
    e->j_abs_max = c.j_abs_max;
    e->clf_scale = c.clf_scale;
    e->clf_problem = c.clf_problem;
    e->clf_bits = c.clf_bits;
    // Sparse matrix?  (route_sparse_dense above.)  Taken when the caller asked for one row read per proposal
    // (field cache OFF), or left the choice (AUTO) on a problem the cached-field sweep cannot serve: where that
    // sweep applies it is the better form while few proposals are accepted (C2b, 1024 replicas, acceptance 2 %:
    // dense int8 rows 7.7e8, as CSR four updates per step 4.3e9, cached fields 1.06e10 attempts/s).
    if (sga_route::sparse_route_wanted(storage, n_models, n, (c.nonint & 1u) == 0u, e->field_cache, e->clf_problem,
                                       e->opt[OPT_SPARSE_ROUTE])) {
        bool taken = false;
        const int rcr = route_sparse_dense(e, src, ld_src, h, n, &taken);  // (h: the caller's pointer)
        if (rcr != SGA_OK || taken) return rcr;
    }
    int rc = pack_dense(e, src, ld_src);
    // row-shared windows on a binary grid (option "row_shared_grid", latched per sweep: the verdict is kept whatever the
    // option says now); a shared-coupling batch: the words, hence k, planes and the bound, are the batch's
    {
        const sga_classify::RsGridVerdict g = sga_classify::row_shared_grid(c);
        e->win.grid_planes = g.why ? 0 : g.planes;
        e->win.grid_k = g.why ? 0 : g.k;
    }
    // The problems the integer cached-field form does not take: which of its conditions failed, and with option
    // "clf_fixed_point" the fixed-point form's verdict (sga_classify.cpp).  After the packing: the diagonal it extracts
    // tells an asymmetric J from a non-zero diagonal -- read back at most once, and only when dE is not consistent.
    if (rc == SGA_OK && !e->clf_problem) {
        int diag_rc = SGA_OK, diag = -1;
        const auto diagonal = [&] {
            if (diag < 0) diag_rc = diag_nonzero(e, rows, &diag);
            return diag == 1;
        };
        if (e->opt[OPT_CLF_FIXED_POINT] == 1) {
            // (option "batch_fixed_point": a many-model batch gets the verdict over its stacked scan -- one k, one width)
            const sga_classify::FxVerdict v =
                sga_classify::dense_fixed_point(c, n_models, diagonal, e->opt[OPT_BATCH_FIXED_POINT] == 1);
            if (diag_rc != SGA_OK) return diag_rc;
            e->clf_fx_why = v.why;
            e->clf_fx_bits = v.bits;
            e->clf_fx_k = v.k;
        }
        const char *why = sga_classify::dense_clf_why(c, diagonal);
        if (diag_rc != SGA_OK) return diag_rc;
        e->clf_why = why;
    }
    if (rc == SGA_OK) rc = ensure_packed(e);
    // the source (the caller's buffer, or the staging copy about to be released) is done with
    HIPCHK(hipStreamSynchronize(e->stream));
    return rc;
}

}  // namespace

extern "C" {

int sga_set_dense(sga_engine *e, const float *J, int64_t ldJ, const float *h, int n, int storage) {
    return set_dense_common(e, J, ldJ, h, n, 1, storage, false);
}

int sga_set_dense_batch(sga_engine *e, const float *J, int64_t ldJ, const float *h, int n,
                        int n_models, int storage) {
    return set_dense_common(e, J, ldJ, h, n, n_models, storage, false);
}

int sga_set_dense_shared(sga_engine *e, const float *J, int64_t ldJ, const float *H, int n, int n_models, int storage) {
    return set_dense_common(e, J, ldJ, H, n, n_models, storage, true);
}

int sga_set_csr(sga_engine *e, const int32_t *rowptr, const int32_t *colidx, const float *val,
                const float *h, int n, int64_t nnz) {
    return set_csr_common(e, rowptr, false, colidx, val, h, n, nnz);
}

int sga_set_csr_shared(sga_engine *e, const int32_t *rowptr, const int32_t *colidx, const float *val, const float *H,
                       int n, int64_t nnz, int n_models) {
    return set_csr_shared(e, rowptr, colidx, val, H, n, nnz, n_models);
}

int sga_set_csr64(sga_engine *e, const int64_t *rowptr, const int32_t *colidx, const float *val,
                  const float *h, int n, int64_t nnz) {
    return set_csr_common(e, rowptr, true, colidx, val, h, n, nnz);
}

int sga_set_tsp(sga_engine *e, const float *dist, int64_t ld, int n_cities, float city_visit,
                float position_fill, const float *h) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (!dist || !h || n_cities < 3 || ld < n_cities) return fail(SGA_ERR_INVALID, "bad TSP problem arguments");
    if (n_cities > 2048) return fail(SGA_ERR_UNSUPPORTED, "more than 2048 cities");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->free_replicas();
    e->free_problem();
    e->opt_stale = 0;
    const int n = n_cities;
    const long long N = (long long)n * n;
    const int waves = (n + 255) / 256, npad = 256 * waves;
    if (sga::tsp_lds_bytes(n, npad) > 160 * 1024 - 256)
        return fail(SGA_ERR_UNSUPPORTED, "replica spins do not fit LDS (too many cities)");
    // the distances on the host (4 MB at 1000 cities): classification of the arithmetic
    std::vector<float> dh((size_t)N), hh((size_t)N);
    HIPCHK(hipMemcpy2D(dh.data(), sizeof(float) * (size_t)n, dist, sizeof(float) * (size_t)ld,
                       sizeof(float) * (size_t)n, (size_t)n, hipMemcpyDefault));
    HIPCHK(hipMemcpy(hh.data(), h, sizeof(float) * (size_t)N, hipMemcpyDefault));
    const float a2 = -(city_visit / 2.0f), b2 = -(position_fill / 2.0f);
    bool integral = a2 == std::rint(a2) && b2 == std::rint(b2);
    sga_classify::BitSpan bits;  // binary exponents of the highest and the lowest set bit of any coupling
    sga_classify::span_add(bits, a2);
    sga_classify::span_add(bits, b2);
    double worst_row = 0.0;
    for (int c = 0; c < n; ++c) {
        double row = 0.0;
        for (int q = 0; q < n; ++q) {
            if (q == c) continue;
            const float v1 = dh[(size_t)c * n + q] / 4.0f, v2 = dh[(size_t)q * n + c] / 4.0f;
            if (!std::isfinite(v1)) return fail(SGA_ERR_INVALID, "distance matrix holds a non-finite value");
            integral = integral && v1 == std::rint(v1);
            sga_classify::span_add(bits, v1);
            row += std::fabs((double)v1) + std::fabs((double)v2);
        }
        worst_row = std::max(worst_row, row);
    }
    for (long long i = 0; i < N && integral; ++i) integral = hh[(size_t)i] == std::rint(hh[(size_t)i]);
    worst_row += (double)(n - 1) * (std::fabs((double)a2) + std::fabs((double)b2));
    const sga_classify::TspClass tc = sga_classify::classify_tsp(bits, integral, worst_row, n);
    const bool exact32 = tc.exact32;
    e->tsp_exact = tc.tsp_exact;
    // site / n by multiply-shift, verified for every site
    const unsigned int magic = (unsigned int)((0x100000000ull + (unsigned long long)n - 1) / (unsigned long long)n);
    for (long long sidx = 0; sidx < N; ++sidx)
        if ((long long)(((unsigned long long)sidx * magic) >> 32) != sidx / n)
            return fail(SGA_ERR_UNSUPPORTED, "internal: site decomposition does not hold for this size");
    // tables on the device
    const float *src = dist;
    long long ld_src = ld;
    struct Staged {
        float *p = nullptr;
        ~Staged() { dev_free(p); }
    } staged;
    if (!is_device_ptr(dist)) {
        HIPCHK(hipMalloc(&staged.p, sizeof(float) * (size_t)N));
        HIPCHK(hipMemcpyAsync(staged.p, dh.data(), sizeof(float) * (size_t)N, hipMemcpyHostToDevice, e->stream));
        src = staged.p;
        ld_src = n;
    }
    HIPCHK(hipMalloc(&e->nd4, sizeof(float) * (size_t)n * npad));
    HIPCHK(hipMalloc(&e->nd4t, sizeof(float) * (size_t)n * npad));
    HIPCHK(sga::launch_tsp_tables(src, ld_src, n, npad, e->nd4, e->nd4t, e->stream));
    HIPCHK(hipMalloc(&e->h, sizeof(float) * (size_t)N));
    HIPCHK(hipMemcpyAsync(e->h, hh.data(), sizeof(float) * (size_t)N, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->tsp = true;
    e->csr = false;
    e->n = (int)N;
    e->n_models = 1;
    e->nnz = 4ll * (n - 1) * N;
    e->consistent_dE = true;  // symmetric with a zero diagonal by construction
    e->table_m = 0;
    e->tsp_waves = waves;
    e->tsp_passes = 1;
    e->tsp_args = sga::TspArgs{e->nd4, e->nd4t, n, npad, magic, (unsigned int)(4 * npad), a2, b2, exact32 ? 0 : 1};
    return SGA_OK;
}

}  // extern "C"

namespace {

// what the remainder of sga_set_groups_csr leaves on the device while it is checked; released on every way out
struct RestStage {
    long long *rowptr64 = nullptr;
    int32_t *rowptr32 = nullptr, *colidx = nullptr;
    float *val = nullptr, *h = nullptr;
    double *row_abs = nullptr;
    int *rptr = nullptr;
    int2 *rent = nullptr;
    ~RestStage() {
        dev_free(rowptr64), dev_free(rowptr32), dev_free(colidx), dev_free(val), dev_free(h), dev_free(row_abs);
        dev_free(rptr), dev_free(rent);
    }
};

// Couplings as a sum of complete graphs on groups, never stored (sweep_groups.hip), plus -- sga_set_groups_csr, nnz > 0 --
// a stored sparse remainder.  The group tables are checked on the host (a few bytes per membership); the remainder is
// scanned where it lies, by the CSR scan kernels of sga_set_csr (extents, columns, diagonal, ordering, symmetry, grid)
// and one pass for sum_j |R_ij| per row.  Then the proof that a combined row sum is exact in fp32 in any order.
// `who`: the call the messages name.
int set_groups_common(sga_engine *e, const char *who_, int n, int n_groups, const int64_t *member_ptr, const int32_t *members,
                      const float *coeff, const int32_t *rowptr, const int32_t *colidx, const float *val, int64_t nnz,
                      const float *h) {
    const std::string who = who_;
    const bool rest = nnz > 0;
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (n <= 0 || !h) return fail(SGA_ERR_INVALID, "bad group problem arguments");
    if (nnz < 0 || (rest && (!rowptr || !colidx || !val))) return fail(SGA_ERR_INVALID, who + ": bad remainder arguments");
    if (n_groups < 0 || (n_groups == 0 && !rest) || (n_groups > 0 && (!member_ptr || !coeff)))
        return fail(SGA_ERR_INVALID, who + ": the extent table is empty (no groups)");
    if (nnz >= (int64_t)INT32_MAX)
        return fail(SGA_ERR_UNSUPPORTED, who + ": the remainder has 2^31 entries or more -- materialise the couplings and use sga_set_csr");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->free_replicas();
    e->free_problem();
    e->opt_stale = 0;
    const size_t G = (size_t)n_groups;
    std::vector<long long> mp(G + 1, 0);
    std::vector<float> cf(G), hh((size_t)n);
    if (G > 0) {
        HIPCHK(hipMemcpy(mp.data(), member_ptr, sizeof(long long) * (G + 1), hipMemcpyDefault));
        HIPCHK(hipMemcpy(cf.data(), coeff, sizeof(float) * G, hipMemcpyDefault));
    }
    HIPCHK(hipMemcpy(hh.data(), h, sizeof(float) * (size_t)n, hipMemcpyDefault));
    if (mp[0] != 0) return fail(SGA_ERR_INVALID, who + ": member_ptr[0] != 0");
    for (size_t q = 0; q < G; ++q)
        if (mp[q + 1] < mp[q]) return fail(SGA_ERR_INVALID, who + ": member_ptr is not monotone at group " + std::to_string(q));
    const long long M = mp[G];
    if (M >= (long long)INT32_MAX) return fail(SGA_ERR_UNSUPPORTED, who + ": 2^31 memberships or more (use sga_set_csr)");
    if (M > 0 && !members) return fail(SGA_ERR_INVALID, "bad group problem arguments");
    std::vector<int32_t> mem((size_t)std::max<long long>(M, 1), 0);
    if (M > 0) HIPCHK(hipMemcpy(mem.data(), members, sizeof(int32_t) * (size_t)M, hipMemcpyDefault));
    // structure: members in range, no site twice in a group; memberships per site
    std::vector<int> count((size_t)n + 1, 0), seen((size_t)n, -1);
    long long max_size = 0;
    for (size_t q = 0; q < G; ++q) {
        if (!std::isfinite(cf[q])) return fail(SGA_ERR_INVALID, who + ": coefficient of group " + std::to_string(q) + " is not finite");
        max_size = std::max(max_size, mp[q + 1] - mp[q]);
        for (long long m = mp[q]; m < mp[q + 1]; ++m) {
            const int i = mem[(size_t)m];
            if (i < 0 || i >= n)
                return fail(SGA_ERR_INVALID, who + ": member " + std::to_string(i) + " of group " + std::to_string(q) +
                                                 " is out of range [0, " + std::to_string(n) + ")");
            if (seen[(size_t)i] == (int)q)
                return fail(SGA_ERR_INVALID, who + ": site " + std::to_string(i) + " is repeated inside group " + std::to_string(q));
            seen[(size_t)i] = (int)q;
            ++count[(size_t)i + 1];
        }
    }
    // the fp32-exact class: every coefficient on one grid 2^-k, 2^k max_i sum_{g contains i} |c_g| (|g| - 1) < 2^24
    sga_classify::BitSpan grid;  // the finest grid any coefficient needs: the lowest set bit of any that contributes a coupling
    for (size_t q = 0; q < G; ++q) sga_classify::groups_span_add(grid, cf[q], mp[q + 1] - mp[q]);
    std::vector<double> bound((size_t)n, 0.0);
    int kmax = 0;
    // the remainder: structure scans on the device (sga_set_csr's kernels), then its grid and sum_j |R_ij| per row
    RestStage rs;
    int rest_max_row = 0, rest_exp_lo = 0;
    if (rest) {
        const size_t np1 = (size_t)n + 1, nz = (size_t)nnz;
        std::vector<int32_t> rp(np1);
        HIPCHK(hipMemcpy(rp.data(), rowptr, sizeof(int32_t) * np1, hipMemcpyDefault));
        HIPCHK(hipMalloc(&rs.rowptr32, sizeof(int32_t) * np1));
        HIPCHK(hipMalloc(&rs.rowptr64, sizeof(long long) * np1));
        HIPCHK(hipMemcpyAsync(rs.rowptr32, rp.data(), sizeof(int32_t) * np1, hipMemcpyHostToDevice, e->stream));
        HIPCHK(sga::launch_widen_rowptr(rs.rowptr32, rs.rowptr64, (long long)np1, e->stream));
        const int32_t *ci = colidx;
        const float *vv = val;
        if (!is_device_ptr(colidx)) {
            HIPCHK(hipMalloc(&rs.colidx, sizeof(int32_t) * nz));
            HIPCHK(hipMemcpyAsync(rs.colidx, colidx, sizeof(int32_t) * nz, hipMemcpyHostToDevice, e->stream));
            ci = rs.colidx;
        }
        if (!is_device_ptr(val)) {
            HIPCHK(hipMalloc(&rs.val, sizeof(float) * nz));
            HIPCHK(hipMemcpyAsync(rs.val, val, sizeof(float) * nz, hipMemcpyHostToDevice, e->stream));
            vv = rs.val;
        }
        HIPCHK(hipMalloc(&rs.h, sizeof(float) * (size_t)n));
        HIPCHK(hipMemcpyAsync(rs.h, hh.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice, e->stream));
        int *d_flags = e->d_flags;
        int flags[sga::CSR_FLAG_COUNT] = {0};
        auto read_flags = [&]() -> hipError_t {
            hipError_t he = hipMemcpyAsync(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, e->stream);
            return he == hipSuccess ? hipStreamSynchronize(e->stream) : he;
        };
        HIPCHK(hipMemsetAsync(d_flags, 0, sizeof(flags), e->stream));
        HIPCHK(sga::launch_csr_check_rowptr(rs.rowptr64, n, nnz, d_flags, e->stream));
        HIPCHK(read_flags());
        if (flags[sga::CSR_BAD_ROWPTR])
            return fail(SGA_ERR_INVALID, who + ": the remainder's rowptr is not monotone or does not span [0, nnz]");
        HIPCHK(sga::launch_csr_scan(rs.rowptr64, ci, vv, rs.h, n, d_flags, e->stream));
        HIPCHK(read_flags());
        if (flags[sga::CSR_BAD_COLUMN])
            return fail(SGA_ERR_INVALID, who + ": a remainder column index is out of range [0, " + std::to_string(n) + ")");
        const std::string way_out = " -- materialise the couplings and use sga_set_csr";
        if (flags[sga::CSR_DIAGONAL])
            return fail(SGA_ERR_UNSUPPORTED, who + ": the remainder has a non-zero diagonal entry" + way_out);
        if (flags[sga::CSR_UNSORTED])
            return fail(SGA_ERR_UNSUPPORTED, who + ": a remainder row is not strictly sorted by column (unsorted or duplicate "
                                                   "entries)" + way_out);
        HIPCHK(sga::launch_csr_symmetry(rs.rowptr64, ci, vv, n, true, d_flags, e->stream));
        HIPCHK(read_flags());
        if (flags[sga::CSR_ASYMMETRIC]) return fail(SGA_ERR_UNSUPPORTED, who + ": the remainder is not symmetric" + way_out);
        for (int i = 0; i < n; ++i) rest_max_row = std::max(rest_max_row, rp[(size_t)i + 1] - rp[(size_t)i]);
        if (rest_max_row > SGA_GROUPS_MAX_REST_ROW) {
            char msg[256];
            std::snprintf(msg, sizeof(msg), "%s: a remainder row has %d entries, more than SGA_GROUPS_MAX_REST_ROW = %d%s", who_,
                          rest_max_row, SGA_GROUPS_MAX_REST_ROW, way_out.c_str());
            return fail(SGA_ERR_UNSUPPORTED, msg);
        }
        rest_exp_lo = flags[sga::CSR_EXP_LO];  // the finest grid any R_ij needs
        HIPCHK(hipMalloc(&rs.row_abs, sizeof(double) * (size_t)n));
        HIPCHK(sga::launch_groups_rest_row_abs(rs.rowptr64, vv, n, rs.row_abs, e->stream));
        HIPCHK(hipMemcpyAsync(bound.data(), rs.row_abs, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
        // the layout the kernels read: 32-bit extents, (column, value bits) interleaved
        HIPCHK(hipMalloc(&rs.rent, sizeof(int2) * nz));
        HIPCHK(sga::launch_pack_cv_rows(rs.rowptr64, rs.rowptr64, ci, vv, nullptr, rs.rent, n, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        for (int i = 0; i < n; ++i)
            if (!std::isfinite(bound[(size_t)i]))
                return fail(SGA_ERR_INVALID, who + ": remainder row " + std::to_string(i) + " holds a value that is not finite");
    }
    for (size_t q = 0; q < G; ++q) {
        const double term = std::fabs((double)cf[q]) * (double)(mp[q + 1] - mp[q] - 1);
        for (long long m = mp[q]; m < mp[q + 1]; ++m) bound[(size_t)mem[(size_t)m]] += term;
    }
    double worst = 0.0;
    for (int i = 0; i < n; ++i) {
        worst = std::max(worst, bound[(size_t)i]);
        kmax = std::max(kmax, count[(size_t)i + 1]);
    }
    const sga_classify::GroupsClass gc = sga_classify::classify_groups(grid, rest_exp_lo, worst);
    const int k = gc.k;
    if (!gc.exact) {
        char msg[320];
        std::snprintf(msg, sizeof(msg),
                      "%s: the couplings are not provably exact in fp32: the coefficients%s lie on the grid 2^%d and "
                      "max_i sum_j |J_ij| = %.6g of its units is not below 2^24 -- materialise them and use sga_set_csr", who_,
                      rest ? " and remainder values" : "", -k, std::ldexp(worst, std::min(k, 126)));
        return fail(SGA_ERR_UNSUPPORTED, msg);
    }
    if (kmax > SGA_GROUPS_MAX_MEMBERSHIPS) {
        char msg[256];
        std::snprintf(msg, sizeof(msg), "%s: a site belongs to %d groups, more than SGA_GROUPS_MAX_MEMBERSHIPS = %d -- "
                      "materialise the couplings and use sga_set_csr", who_, kmax, SGA_GROUPS_MAX_MEMBERSHIPS);
        return fail(SGA_ERR_UNSUPPORTED, msg);
    }
    {
        sga_route_query q;
        (void)sga_route_query_init(&q);
        q.kind = SGA_ROUTE_GROUPS;
        q.n = n;
        q.n_groups = n_groups;
        q.group_max = (int32_t)max_size;
        const sga_route::GroupsForm f = sga_route::groups_form(q);
        if (f.error) return fail(SGA_ERR_UNSUPPORTED, who + ": " + f.error + " -- use sga_set_csr");
    }
    // site -> group table, groups of a site in group order; one zero entry behind (the kernels' padding entry)
    std::vector<int> gptr((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) gptr[(size_t)i + 1] = gptr[(size_t)i] + count[(size_t)i + 1];
    std::vector<int2> gent((size_t)M + 1, make_int2(0, 0));
    std::vector<int> cur(gptr.begin(), gptr.end() - 1);
    for (size_t q = 0; q < G; ++q) {
        int cbits;
        std::memcpy(&cbits, &cf[q], sizeof(cbits));
        for (long long m = mp[q]; m < mp[q + 1]; ++m) gent[(size_t)cur[(size_t)mem[(size_t)m]]++] = make_int2((int)q, cbits);
    }
    HIPCHK(hipMalloc(&e->g_gptr, sizeof(int) * ((size_t)n + 1)));
    HIPCHK(hipMalloc(&e->g_gent, sizeof(int2) * ((size_t)M + 1)));
    HIPCHK(hipMalloc(&e->g_member_ptr, sizeof(long long) * (G + 1)));
    HIPCHK(hipMalloc(&e->g_members, sizeof(int) * (size_t)std::max<long long>(M, 1)));
    HIPCHK(hipMalloc(&e->g_coeff, sizeof(float) * std::max<size_t>(G, 1)));
    HIPCHK(hipMalloc(&e->h, sizeof(float) * (size_t)n));
    HIPCHK(hipMemcpyAsync(e->g_gptr, gptr.data(), sizeof(int) * ((size_t)n + 1), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->g_gent, gent.data(), sizeof(int2) * ((size_t)M + 1), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->g_member_ptr, mp.data(), sizeof(long long) * (G + 1), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->g_members, mem.data(), sizeof(int) * mem.size(), hipMemcpyHostToDevice, e->stream));
    if (G > 0) HIPCHK(hipMemcpyAsync(e->g_coeff, cf.data(), sizeof(float) * G, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->h, hh.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->groups = true;
    e->csr = false;
    e->n = n;
    e->n_models = 1;
    long long pairs = 0;
    for (size_t q = 0; q < G; ++q) pairs += (mp[q + 1] - mp[q]) * (mp[q + 1] - mp[q] - 1);
    e->nnz = pairs + nnz;  // entries of the materialised couplings, overlaps counted once per group (and per remainder entry)
    e->consistent_dE = true;  // symmetric with a zero diagonal by construction
    e->table_m = 0;
    e->g_memberships = M;
    e->g_max_size = (int)max_size;
    e->g_kmax = kmax;
    e->g_exp = k;
    e->group_args = sga::GroupArgs{e->g_gptr, e->g_gent, e->g_member_ptr, e->g_members, n_groups, max_size >= (1 << 15) ? 1 : 0,
                                   {nullptr, nullptr, 0, 0}};
    if (rest) {  // the staged layout becomes the engine's
        e->g_rptr = reinterpret_cast<int *>(rs.rowptr32);
        e->g_rent = rs.rent;
        rs.rowptr32 = nullptr;
        rs.rent = nullptr;
        e->group_args.rest = sga::GroupArgs::Rest{e->g_rptr, e->g_rent, (long long)nnz, rest_max_row};
    }
    return SGA_OK;
}

}  // namespace

extern "C" {

int sga_set_groups(sga_engine *e, int n, int n_groups, const int64_t *member_ptr, const int32_t *members, const float *coeff,
                   const float *h) {
    if (n_groups <= 0 || !member_ptr || !coeff) {
        if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
        if (n <= 0 || !h) return fail(SGA_ERR_INVALID, "bad group problem arguments");
        return fail(SGA_ERR_INVALID, "sga_set_groups: the extent table is empty (no groups)");
    }
    return set_groups_common(e, "sga_set_groups", n, n_groups, member_ptr, members, coeff, nullptr, nullptr, nullptr, 0, h);
}

int sga_set_groups_csr(sga_engine *e, int n, int n_groups, const int64_t *member_ptr, const int32_t *members, const float *coeff,
                       const int32_t *rowptr, const int32_t *colidx, const float *val, int64_t nnz, const float *h) {
    return set_groups_common(e, "sga_set_groups_csr", n, n_groups, member_ptr, members, coeff, rowptr, colidx, val, nnz, h);
}

// Ragged CSR batches: M independent problems of any sizes in one engine, their rows concatenated (model m owns rows
// [row0_m, row0_m + n_m), its columns model-local).  Each model gets sga_set_csr's structure checks -- the same scan
// kernels over the model's rows (extents offset to its first row, columns bounded by its n) -- and its own class;
// the batch runs the most general accumulation class and the widest accept table any model needs (why every model's
// chain stays exact: sweep_csr_impl.h, RAGGED).  The layout is the plain (column, value) one: the narrow one-update
// form is the only one built for ragged batches.
int sga_set_csr_batch(sga_engine *e, int n_models, const int32_t *n_spins, const int64_t *rowptr,
                      const int32_t *colidx, const float *val, const float *h, int64_t nnz) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (n_models <= 0 || !n_spins || !rowptr || !h || nnz < 0 || (nnz > 0 && (!colidx || !val)))
        return fail(SGA_ERR_INVALID, "bad CSR batch arguments");
    if (is_device_ptr(n_spins)) return fail(SGA_ERR_INVALID, "n_spins must be a host array");
    long long total = 0;
    int n_max = 0;
    for (int m = 0; m < n_models; ++m) {
        if (n_spins[m] <= 0) return fail(SGA_ERR_INVALID, "model " + std::to_string(m) + ": n_spins <= 0");
        total += n_spins[m];
        n_max = std::max(n_max, (int)n_spins[m]);
    }
    if (total >= (long long)INT32_MAX || nnz + CSR_TAIL_PAD >= (int64_t)INT32_MAX)
        return fail(SGA_ERR_UNSUPPORTED, "CSR batch needs 64-bit row extents (ragged batches run the narrow form, "
                                         "32-bit extents only)");
    if (sga::csr_waves_per_block((n_max + 15) / 16 * 16, 0) < 1)
        return fail(SGA_ERR_UNSUPPORTED, "CSR batch: the largest model (" + std::to_string(n_max) +
                                             " spins) does not fit the narrow int8 form's LDS slice");
    const int N = (int)total;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->free_replicas();
    e->free_problem();
    e->opt_stale = 0;
    e->csr = true;
    e->from_dense = false;
    e->n = N;  // (rows, while the layout is built; the largest model's spins below)
    e->n_models = n_models;
    e->nnz = nnz;
    const size_t np1 = (size_t)N + 1;
    auto bail = [&](int code, const std::string &msg) {
        (void)hipStreamSynchronize(e->stream);
        dev_free(e->colidx);
        dev_free(e->val);
        e->free_problem();
        return fail(code, msg);
    };
    auto check = [&](hipError_t he) -> int {
        return he == hipSuccess ? SGA_OK : bail(he == hipErrorOutOfMemory ? SGA_ERR_MEMORY : SGA_ERR_DEVICE, hipGetErrorString(he));
    };
#define SGA_BATCH_CHK(expr)                  \
    do {                                     \
        const int _rc = check(expr);         \
        if (_rc != SGA_OK) return _rc;       \
    } while (0)
    SGA_BATCH_CHK(hipMalloc(&e->rowptr64, sizeof(long long) * np1));
    SGA_BATCH_CHK(hipMemcpyAsync(e->rowptr64, rowptr, sizeof(long long) * np1, hipMemcpyDefault, e->stream));
    const size_t nz = (size_t)std::max<int64_t>(nnz, 1);
    const int32_t *ci = colidx;
    const float *vv = val;
    if (nnz > 0 && !is_device_ptr(colidx)) {
        SGA_BATCH_CHK(hipMalloc(&e->colidx, sizeof(int32_t) * nz));
        SGA_BATCH_CHK(hipMemcpyAsync(e->colidx, colidx, sizeof(int32_t) * nz, hipMemcpyHostToDevice, e->stream));
        ci = e->colidx;
    }
    if (nnz > 0 && !is_device_ptr(val)) {
        SGA_BATCH_CHK(hipMalloc(&e->val, sizeof(float) * nz));
        SGA_BATCH_CHK(hipMemcpyAsync(e->val, val, sizeof(float) * nz, hipMemcpyHostToDevice, e->stream));
        vv = e->val;
    }
    // h, then the model table {first row, spins} 8-byte aligned behind it (SweepArgs::ragged: the sweep kernel finds
    // it through h)
    const int h_floats = (N + 1) & ~1;
    SGA_BATCH_CHK(hipMalloc(&e->h, sizeof(float) * (size_t)h_floats + sizeof(int2) * (size_t)n_models));
    SGA_BATCH_CHK(hipMemcpyAsync(e->h, h, sizeof(float) * (size_t)N, hipMemcpyDefault, e->stream));
    e->d_models = reinterpret_cast<int2 *>(e->h + h_floats);
    SGA_BATCH_CHK(hipMalloc(&e->diag, sizeof(float) * (size_t)N));
    SGA_BATCH_CHK(hipMemsetAsync(e->diag, 0, sizeof(float) * (size_t)N, e->stream));  // (a diagonal is refused below)

    int flags[sga::CSR_FLAG_COUNT] = {0};
    auto scan = [&](auto &&launch) -> hipError_t {
        hipError_t he = hipMemsetAsync(e->d_flags, 0, sizeof(flags), e->stream);
        if (he == hipSuccess) he = launch();
        if (he == hipSuccess) he = hipMemcpyAsync(flags, e->d_flags, sizeof(flags), hipMemcpyDeviceToHost, e->stream);
        return he == hipSuccess ? hipStreamSynchronize(e->stream) : he;
    };
    SGA_BATCH_CHK(scan([&] { return sga::launch_csr_check_rowptr(e->rowptr64, N, nnz, e->d_flags, e->stream); }));
    if (flags[sga::CSR_BAD_ROWPTR])
        return bail(SGA_ERR_INVALID, "CSR batch rowptr is not monotone or does not span [0, nnz]");
    std::vector<long long> src(np1);
    SGA_BATCH_CHK(hipMemcpyAsync(src.data(), e->rowptr64, sizeof(long long) * np1, hipMemcpyDeviceToHost, e->stream));
    SGA_BATCH_CHK(hipStreamSynchronize(e->stream));

    // per model: the scans of sga_set_csr, then its class (force_csr_acc applies to the batch); sga_classify::fold_ragged
    // takes the most general class and the widest table, and names the first model that keeps the batch off the
    // cached-field forms (options "ragged_field_cache", "clf_fixed_point"; sga_sweep under SGA_FIELD_CACHE_ON reports it)
    std::vector<sga_classify::CsrClass> classes((size_t)n_models);
    std::vector<int> row0((size_t)n_models);
    std::vector<int2> models((size_t)n_models);
    for (int m = 0, r0 = 0; m < n_models; r0 += n_spins[m], ++m) {
        const int nm = n_spins[m];
        row0[(size_t)m] = r0;
        models[(size_t)m] = make_int2(r0, nm);
        const std::string who = "model " + std::to_string(m) + ": ";
        SGA_BATCH_CHK(scan([&] { return sga::launch_csr_scan(e->rowptr64 + r0, ci, vv, e->h + r0, nm, e->d_flags, e->stream); }));
        if (flags[sga::CSR_BAD_COLUMN])
            return bail(SGA_ERR_INVALID, who + "CSR column index out of range [0, " + std::to_string(nm) + ")");
        if (flags[sga::CSR_NOT_INTEGRAL] & sga::SCAN_NON_FINITE) return bail(SGA_ERR_INVALID, who + NON_FINITE_MSG);
        if (flags[sga::CSR_DIAGONAL])
            return bail(SGA_ERR_UNSUPPORTED, who + "non-zero diagonal entry (ragged CSR batches need a zero diagonal)");
        const bool sorted = !flags[sga::CSR_UNSORTED];
        const long long mnnz = src[(size_t)r0 + nm] - src[(size_t)r0];
        const double avg_deg = (double)mnnz / nm;
        int sym[sga::CSR_FLAG_COUNT];
        std::memcpy(sym, flags, sizeof(sym));
        if (sorted || (double)mnnz * avg_deg <= 4.0e10) {
            SGA_BATCH_CHK(scan([&] { return sga::launch_csr_symmetry(e->rowptr64 + r0, ci, vv, nm, sorted, e->d_flags, e->stream); }));
            sym[sga::CSR_ASYMMETRIC] = flags[sga::CSR_ASYMMETRIC];
        } else {
            sym[sga::CSR_ASYMMETRIC] = 1;
        }
        if (sym[sga::CSR_ASYMMETRIC])
            return bail(SGA_ERR_UNSUPPORTED, who + "asymmetric J (ragged CSR batches need J[i][j] == J[j][i])");
        long long max_len = 0;
        for (int i = r0; i < r0 + nm; ++i) max_len = std::max(max_len, src[(size_t)i + 1] - src[(size_t)i]);
        classes[(size_t)m] = sga_classify::classify_csr(csr_scan_of(sym), max_len, nm, {e->opt[OPT_HALF_TABLE] != 0, 0});
        keep_csr_scan(e, sym, max_len);
    }
    const bool want_clf = e->opt[OPT_RAGGED_FIELD_CACHE] == 1;
    const sga_classify::RaggedClass b = sga_classify::fold_ragged(
        classes, {(int)e->opt[OPT_FORCE_CSR_ACC], want_clf, want_clf && e->opt[OPT_CLF_FIXED_POINT] == 1});
    e->csr_acc = b.acc;
    e->csr_x_exact = false;  // (no all-replica pass over ragged batches)
    e->table_scale = b.table_scale;
    e->table_m = b.table_m;
    e->csr_row_abs_max = b.row_abs_max;
    e->csr_sorted = b.sorted;
    e->consistent_dE = true;
    e->row_j_abs_max = b.row_j_abs_max;
    e->clf_csr_problem = b.clf_problem;
    e->clf_ragged_why = b.clf_why;
    e->clf_fx_bits = b.fx_bits;
    e->clf_fx_k = b.fx_k;
    // the plain layout: (column, value) interleaved, CSR_TAIL_PAD zeroed entries behind
    long long *src_ptr = nullptr;
    SGA_BATCH_CHK(hipMalloc(&src_ptr, sizeof(long long) * np1));
    hipError_t he = hipMemcpyAsync(src_ptr, e->rowptr64, sizeof(long long) * np1, hipMemcpyDeviceToDevice, e->stream);
    int rc = he == hipSuccess ? build_layout(e, src, false) : fail(SGA_ERR_DEVICE, hipGetErrorString(he));
    if (rc == SGA_OK) {
        he = hipMalloc(&e->cv, sizeof(int2) * (size_t)(e->layout_entries + CSR_TAIL_PAD));
        if (he == hipSuccess) he = hipMemsetAsync(e->cv + e->layout_entries, 0, sizeof(int2) * CSR_TAIL_PAD, e->stream);
        if (he == hipSuccess) he = sga::launch_pack_cv_rows(src_ptr, e->rowptr64, ci, vv, nullptr, e->cv, N, e->stream);
        if (he == hipSuccess)
            he = hipMemcpyAsync(e->d_models, models.data(), sizeof(int2) * (size_t)n_models, hipMemcpyHostToDevice, e->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
        if (he != hipSuccess) rc = fail(he == hipErrorOutOfMemory ? SGA_ERR_MEMORY : SGA_ERR_DEVICE, hipGetErrorString(he));
    }
    dev_free(src_ptr);
    dev_free(e->colidx);
    dev_free(e->val);
    if (rc != SGA_OK) {
        const std::string msg = g_last_error;
        e->free_problem();
        return fail(rc, msg);
    }
#undef SGA_BATCH_CHK
    e->ragged = true;
    e->ragged_at = h_floats;
    e->n_rows = N;
    e->n = n_max;
    e->model_n.assign(n_spins, n_spins + n_models);
    e->model_row0 = row0;
    return SGA_OK;
}

int sga_get_scan_summary(sga_engine *e, int model, int32_t *kind, int32_t *words, int capacity, int *count) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (e->n <= 0) return fail(SGA_ERR_INVALID, "no problem set");
    if (e->implicit() || e->scan_words.empty() || e->scan_per_model <= 0)
        return fail(SGA_ERR_UNSUPPORTED, "sga_get_scan_summary: implicit couplings (sga_set_tsp, sga_set_groups*) are scanned on "
                                         "the host and keep no scan words");
    const int models = (int)(e->scan_words.size() / (size_t)e->scan_per_model);
    if (model < 0 || model >= models)
        return fail(SGA_ERR_INVALID, e->csr ? "model index out of range" : "a dense batch is scanned stacked: model must be 0");
    if (count) *count = e->scan_per_model;
    if (kind) *kind = e->csr ? SGA_ROUTE_CSR : SGA_ROUTE_DENSE;
    if (words) {
        if (capacity < e->scan_per_model) return fail(SGA_ERR_INVALID, "sga_get_scan_summary: capacity below the word count");
        std::memcpy(words, e->scan_words.data() + (size_t)model * e->scan_per_model, sizeof(int32_t) * (size_t)e->scan_per_model);
    }
    return SGA_OK;
}

int sga_get_batch_model(sga_engine *e, int m, int *n_spins, int *first_replica, int *n_replicas) {
    if (!e) return fail(SGA_ERR_INVALID, "engine is NULL");
    if (!e->ragged) return fail(SGA_ERR_INVALID, "not a ragged CSR batch (sga_set_csr_batch)");
    if (m < 0 || m >= e->n_models) return fail(SGA_ERR_INVALID, "model index out of range");
    if (n_spins) *n_spins = e->model_n[(size_t)m];
    const int reps = e->Rg > 0 ? e->Rg / e->n_models : 0;
    if (first_replica) *first_replica = m * reps;
    if (n_replicas) *n_replicas = reps;
    return SGA_OK;
}

}  // extern "C"
