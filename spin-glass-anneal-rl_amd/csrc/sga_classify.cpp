// sga_classify.cpp -- which arithmetic a problem admits (sga_classify.h).  Host arithmetic on scan summaries only.
#include "sga_classify.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace sga_classify {

void span_add(BitSpan &s, float v) {
    if (v == 0.0f || !std::isfinite(v)) return;
    int ex;
    const float m = std::frexp(std::fabs(v), &ex);  // v = m 2^ex, m in [0.5, 1)
    uint32_t mant = (uint32_t)std::ldexp(m, 24);    // 24-bit integer mantissa
    int low = 0;
    while (!(mant & 1u)) {
        mant >>= 1;
        ++low;
    }
    s.hi = std::max(s.hi, ex - 1);
    s.lo = std::min(s.lo, ex - 24 + low);
    s.any = true;
}

BitSpan span_of_words(int hi_word, int lo_word) {
    BitSpan s;
    s.any = hi_word != 0;
    if (s.any) s.hi = hi_word - 1024, s.lo = 1024 - lo_word;
    return s;
}

int carry_bits(long long terms) {
    int carry = 0;
    while ((1ll << carry) < std::max<long long>(terms, 1)) ++carry;
    return carry;
}

// How exact is a row sum?  Integer J with sum |J| < 2^24: fp32 accumulation is exact.  Else,
// if every J's set bits lie within 53 binary places of each other once the carries of
// the longest row are counted, the fp64 sum of the (exact) fp32 products is exact in any
// order.  Only couplings of a wider dynamic range (e.g. Gaussian J: tiny values next to large ones) need the
// canonical summation order.  `terms`: the longest CSR row; n of a dense row; 4 n cities of a TSP site -- kept as found.
bool fp64_exact_any_order(const BitSpan &s, long long terms) { return !s.any || s.hi - s.lo + 1 + carry_bits(terms) <= 52; }

// (field_max is the fp32 rounding of an fp64 sum: < 1 ulp either way)
double fx_bound(double field_max, int k) { return std::ldexp(field_max, k) * (1.0 + 0x1.0p-20); }

// Option "clf_fixed_point": the cached-field sweep for the problems the integer forms do not take.  Every row sum is
// exact (acc classes f32 / f64-exact), and every set bit of every J lies at or above 2^-k, k = minus the exponent of the
// lowest set bit (0 for integer J where clamped): D_i = 2^k sum_j J_ij s_j is an integer of at most B = 2^k max_i sum_j
// |J_ij| (< 2^53 by the class's own bound), kept exactly as int32 (B < 2^31) or int64.  h is never folded in.
FxVerdict fixed_point_verdict(const FxQuery &q, const std::function<bool()> &diagonal) {
    FxVerdict v;
    const int k = q.span.any ? (q.clamp_k ? std::max(-q.span.lo, 0) : -q.span.lo) : 0;
    const double bound = fx_bound(q.field_max, k);
    if (q.batch)
        v.why = "cached local fields (fixed point): not built for dense batches (one model only)";
    else if (q.canonical)
        v.why = q.stacked ? "cached local fields (fixed point): the couplings need the canonical fp64 summation order "
                            "(acc class f64-canonical: their binary places span more than 53 bits over the stack, so no "
                            "exact fixed point at one k holds a row sum; a dense batch: in every model)"
                          : "cached local fields (fixed point): the couplings need the canonical fp64 summation order "
                            "(acc class f64-canonical: their binary places span more than 53 bits, so no exact fixed "
                            "point holds a row sum)";
    else if (q.unsorted)
        v.why = "cached local fields (fixed point): CSR rows must be strictly sorted by column (no duplicate entries)";
    else if (!q.consistent_dE)
        v.why = diagonal() ? (q.stacked ? "cached local fields (fixed point): J must have a zero diagonal (a dense batch: in every model)"
                                        : "cached local fields (fixed point): J must have a zero diagonal")
                           : (q.stacked ? "cached local fields (fixed point): J must be symmetric (a dense batch: in every model)"
                                        : "cached local fields (fixed point): J must be symmetric");
    else if (q.n_too_large || !(bound < FX_LIMIT_ONE))
        v.why = q.stacked ? "cached local fields (fixed point): fields wider than int64 (a dense batch: in every model, at the "
                            "batch-wide k)"
                          : "cached local fields (fixed point): fields wider than int64";
    else
        v.bits = fx_bits(bound), v.k = k;
    return v;
}

CsrClass classify_csr(const CsrScan &s, long long longest_row, int n, const CsrOptions &o) {
    CsrClass c;
    c.scan = s;
    c.longest_row = longest_row;
    c.span = span_of_words(s.exp_hi_word, s.exp_lo_word);
    c.sorted = !s.unsorted;
    c.consistent_dE = !s.asymmetric && !s.diagonal;
    // integer-valued problem?  then dE takes at most M = max_i(sum_j |J_ij| + |h_i|) even values
    // (J integer, h a multiple of 1/2 -- penalty encodings of 0/1 variables: dE takes integer values,
    // tabulated at twice the resolution)
    const float m = c.row_abs_max = s.row_abs_max, mj = c.row_j_abs_max = s.row_j_abs_max;
    if (!s.not_integral && m >= 1.0f && m < 16777216.0f) {
        c.table_m = (int)std::min(m, 2048.0f);
    } else if ((s.not_integral & 5) == 0 && m >= 1.0f && m < 8388608.0f && o.half_integer_table) {
        c.table_m = (int)std::min(2.0f * m, 2048.0f);
        c.table_scale = 2;
    }
    // cached-field sweep over CSR: exact int16 dynamic fields, table arithmetic, every entry its own column
    c.clf_int16 = (s.not_integral & 5) == 0 && c.table_m > 0 && c.consistent_dE && c.sorted && mj < 32768.0f && n <= (1 << 30);
    if ((s.not_integral & 1) == 0 && m < 16777216.0f)
        c.acc = c.table_m > 0 ? ACC_F32_TABLE : ACC_F32;
    else
        c.acc = fp64_exact_any_order(c.span, longest_row) ? ACC_F64 : ACC_F64_CANON;
    if (o.force_csr_acc > 0) c.acc = std::max(c.acc, std::min(3, o.force_csr_acc));  // parity tests: the slower forms
    // Is X = sum_i mv_i s_i exact in fp64 in any order?  Every row sum is exact (classes f32 / f64-exact) and a
    // multiple of 2^e_lo, so is its fp32 rounding mv_i; every partial sum of X is at most n max_i sum_j |J_ij|
    // (mj: an fp32 rounding, < 1 ulp either way).  Then the all-replica pass's group order gives the bits of the
    // per-replica kernels' order (recompute_energy_range).
    c.x_exact = c.acc != ACC_F64_CANON && (!c.span.any || std::ldexp((double)n * (double)mj * (1.0 + 0x1.0p-20), -c.span.lo) < 0x1.0p53);
    return c;
}

FxVerdict csr_fixed_point(const CsrClass &c, int n) {
    FxQuery q;
    q.span = c.span;
    q.clamp_k = false;                // kept as found: k of CSR couplings is not clamped at 0 (dense: clamped)
    q.field_max = c.row_j_abs_max;    // kept as found: max_i sum_j |J_ij| (dense: with |h_i|)
    q.canonical = c.acc == ACC_F64_CANON;
    q.unsorted = !c.sorted;
    q.consistent_dE = c.consistent_dE;
    q.n_too_large = n > (1 << 30);    // kept as found: a condition of CSR only
    return fixed_point_verdict(q, [&] { return c.scan.diagonal; });
}

// The batch runs the most general accumulation class and the widest accept table any model needs.  Cached fields: per
// model the int16 conditions of classify_csr and rows of <= 2048 entries; the fixed-point form per model the class of its
// row sums, sorted rows, rows of <= 2048 entries, and batch-wide k = the finest grid any model needs with 2^k max_i sum_j
// |J_ij| over all rows picking the width.  Either reason names the first offending model.
RaggedClass fold_ragged(const std::vector<CsrClass> &models, const RaggedOptions &o) {
    RaggedClass b;
    std::string fx_why;
    int scale_b = 1, fx_k = INT_MIN;
    for (size_t m = 0; m < models.size(); ++m) {
        const CsrClass &c = models[m];
        const std::string who = "model " + std::to_string(m) + ": ";
        b.sorted = b.sorted && c.sorted;
        b.acc = std::max(b.acc, c.acc);
        if (c.acc == ACC_F32_TABLE) scale_b = std::max(scale_b, c.table_scale);
        b.row_abs_max = std::max(b.row_abs_max, c.row_abs_max);
        b.row_j_abs_max = std::max(b.row_j_abs_max, c.row_j_abs_max);
        if (o.want_clf && b.clf_why.empty()) {
            const char *bad = nullptr;
            if (c.scan.not_integral & 1) bad = "J is not integer valued";
            else if (c.scan.not_integral & 4) bad = "h is not a multiple of 1/2";
            else if (!c.sorted) bad = "rows are not strictly sorted by column (unsorted or duplicate entries)";
            else if (!(c.row_j_abs_max < 32768.0f)) bad = "max_i sum_j |J_ij| is not below 2^15 (int16 fields)";
            else if (c.longest_row > 4 * 64 * 8) bad = "a row is longer than 2048 entries";
            else if (c.acc != ACC_F32_TABLE)
                bad = "the accept table does not apply (max_i (sum_j |J_ij| + |h_i|) outside [1, 2^24), or half-integer h with "
                      "option \"half_integer_table\" = 0)";
            if (bad) b.clf_why = "cached local fields over ragged CSR batches: " + who + bad;
        }
        if (o.want_fx) {
            if (c.span.any) fx_k = std::max(fx_k, -c.span.lo);  // k_m: minus the exponent of J's lowest set bit
            const char *bad = nullptr;
            if (c.acc == ACC_F64_CANON)
                bad = "the couplings need the canonical fp64 summation order (acc class f64-canonical: their binary places span "
                      "more than 53 bits, so no exact fixed point holds a row sum)";
            else if (!c.sorted) bad = "rows are not strictly sorted by column (unsorted or duplicate entries)";
            else if (c.longest_row > 4 * 64 * 8) bad = "a row is longer than 2048 entries";
            if (bad && fx_why.empty()) fx_why = "cached local fields over ragged CSR batches (fixed point): " + who + bad;
        }
    }
    if (o.force_csr_acc > 0) b.acc = std::max(b.acc, std::min(3, o.force_csr_acc));
    b.table_scale = b.acc == ACC_F32_TABLE ? scale_b : 1;
    b.table_m = b.acc == ACC_F32_TABLE ? (int)std::min((double)b.table_scale * b.row_abs_max, 2048.0) : 0;
    if (o.want_clf && b.clf_why.empty() && (b.acc != ACC_F32_TABLE || b.table_m <= 0))
        b.clf_why = "cached local fields over ragged CSR batches: the batch runs without an accept table (option \"force_csr_acc\")";
    b.clf_problem = o.want_clf && b.clf_why.empty();
    if (!o.want_clf) b.clf_why.clear();
    if (o.want_fx && !b.clf_why.empty()) {  // the int16 form does not take the batch: the fixed-point form
        const int k = fx_k == INT_MIN ? 0 : fx_k;
        // D_i = 2^k sum_j J_ij s_j of any row of the batch must stay below 2^53: then the fp64 sums of the seed kernel, the
        // int64 -> fp64 conversion of a proposal and the scaled entries of an accept are all exact (the one-model condition
        // over the concatenation; mj is the fp32 rounding of an fp64 sum: < 1 ulp either way)
        double bound = 0.0;
        for (size_t m = 0; m < models.size(); ++m) {
            const double bm = fx_bound((double)models[m].row_j_abs_max, k);
            bound = std::max(bound, bm);
            if (fx_why.empty() && !(bm < FX_LIMIT_RAGGED)) {
                char msg[256];
                std::snprintf(msg, sizeof(msg), "cached local fields over ragged CSR batches (fixed point): model %d: fields wider "
                              "than the bound: 2^k max_i sum_j |J_ij| is not below 2^53 at the batch-wide k = %d", (int)m, k);
                fx_why = msg;
            }
        }
        if (fx_why.empty() && b.acc == ACC_F64_CANON)
            fx_why = "cached local fields over ragged CSR batches (fixed point): the batch runs the canonical fp64 summation order "
                     "(option \"force_csr_acc\")";
        b.clf_problem = fx_why.empty();
        if (b.clf_problem) b.fx_bits = fx_bits(bound), b.fx_k = k;
        b.clf_why = fx_why;
    }
    return b;
}

DenseClass classify_dense(const int hflags[8], int n, int n_models, int storage, bool force_dense_canonical) {
    DenseClass c;
    c.consistent_dE = hflags[4] == 0;
    c.fits_i8 = hflags[0] == 0;
    c.ternary = hflags[1] == 0 && n_models == 1;
    c.use_t2 = storage == SGA_J_T2 || (storage == SGA_J_AUTO && c.ternary && n >= 4096);
    c.want_i8 = c.use_t2 || (storage == SGA_J_I8) || (storage == SGA_J_AUTO && c.fits_i8);
    float m, jm;
    std::memcpy(&m, &hflags[2], sizeof(float));
    std::memcpy(&jm, &hflags[7], sizeof(float));  // max |J_ij| as float bits
    c.nonint = (unsigned)hflags[3];
    // fp32 partial sums are exact (any order) when J is integer valued and no row's sum of
    // |J| reaches 2^24; otherwise the row sum is accumulated in fp64 -- in the canonical summation order and its one
    // tree per 256-element chunk only where fp64_exact_any_order does not hold
    c.acc64 = !c.want_i8 && !((c.nonint & 1u) == 0u && m < 16777216.0f);
    c.span = span_of_words(hflags[5], hflags[6]);
    c.acc_canon = c.acc64 && !fp64_exact_any_order(c.span, n);
    if (force_dense_canonical) c.acc_canon = c.acc64;  // parity tests
    // integer problem: tabulate exp(float32(-2k/T)) for the moves k <= min(M, 2048) per sweep
    if (c.nonint == 0u && m >= 1.0f && m < 16777216.0f) c.table_m = (int)std::min(m, 2048.0f);
    // cached-local-field sweep: exact integer fields, dE of the rule == energy change
    // (h a multiple of 1/2 -- the penalty encodings of 0/1 variables -- keeps 2 F an integer: scale 2).  A many-model
    // batch qualifies as a whole: the scans above run over all stacked rows, so scale, field width, accept table and
    // max |J| are batch-wide -- a field kept at scale 2 or as int32 because ANOTHER model needs it is still exact
    c.row_abs_max = m;
    c.j_max = jm;
    c.j_abs_max = (int)std::min(std::ceil((double)jm), 16777216.0);
    c.clf_scale = (c.nonint & 2u) ? 2 : 1;
    c.clf_problem = (c.nonint & 5u) == 0u && (double)m * c.clf_scale < 16777216.0 && c.consistent_dE;
    c.clf_bits = (double)m * c.clf_scale < 32768.0 ? 16 : 32;
    return c;
}

// (the route query carries only the verdict); a batch is scanned as a whole, so the reason names what SOME model does
const char *dense_clf_why(const DenseClass &c, const std::function<bool()> &diagonal) {
    if (c.nonint & 1u) return "cached local fields: J must be integer valued (a dense batch: in every model)";
    if (c.nonint & 4u) return "cached local fields: h must be in multiples of 1/2 (a dense batch: in every model)";
    if (!c.consistent_dE)
        return diagonal() ? "cached local fields: J must have a zero diagonal (a dense batch: in every model)"
                          : "cached local fields: J must be symmetric (a dense batch: in every model)";
    return "cached local fields: max_i (sum_j |J_ij| + |h_i|) must stay below 2^24 (2^23 with half-integer h)";
}

// (sweep_clf_fx.hip; bit-plane problems are served from their int8 rows)
// Many-model batches (batch_allowed: option "batch_fixed_point"): the one-model verdict over the STACKED scan.  The span
// is over every model's J, so k is the finest grid any model needs and every model's 2^k J is an integer; the class
// (fp32-exact / f64-exact) and the field bound hold over all stacked rows, so every row sum of every model is exact
// and dot = fp32(2^-k D_i) is the one rounding of that exact sum -- the value the row kernels form for that model
// alone, whatever class, k or width the model would get on its own.  Every model walks its one-model chain.
FxVerdict dense_fixed_point(const DenseClass &c, int n_models, const std::function<bool()> &diagonal, bool batch_allowed) {
    FxQuery q;
    q.span = c.span;
    q.clamp_k = true;              // kept as found: dense k is clamped at 0 (CSR: not)
    q.field_max = c.row_abs_max;   // kept as found: max_i (sum_j |J_ij| + |h_i|) bounds max_i sum_j |J_ij| from above (CSR: without h)
    q.batch = n_models != 1 && !batch_allowed;
    q.stacked = n_models != 1 && batch_allowed;
    q.canonical = c.acc_canon;
    q.consistent_dE = c.consistent_dE;
    return fixed_point_verdict(q, diagonal);
}

// Every J_ij is an integer multiple of 2^-k (k = minus the exponent of the lowest set bit of any J, clamped at 0 as
// dense_fixed_point clamps it), so the planes of 2^k J are integer planes; a row sum is 2^-k times an integer D with
// |D| <= 2^k max_i sum_j |J_ij| < 2^24 (row_abs_max, which includes |h_i|, bounds that maximum from above; fx_bound
// allows for its fp32 rounding), so every partial sum is exact in fp32 in any order and fp32(2^-k D) is the row
// kernels' dot.  h stays outside the sums: any finite fp32 value.  The planes follow sga::row_shared_planes
// (sga_kernels.h) on the scaled maximum -- 1 | 3 | 8 for up to 1 | 7 | 255 -- written out here: this file calls no
// kernel header.
RsGridVerdict row_shared_grid(const DenseClass &c) {
    RsGridVerdict v;
    const int k = c.span.any ? std::max(0, -c.span.lo) : 0;
    const double scaled = k <= RS_GRID_MAX_K ? std::ldexp((double)c.j_max, k) : 0.0;
    if (c.table_m > 0 && !c.acc64)
        v.why = "row-shared windows (grid): an integer problem, the integer form of the windows serves it";
    else if (!c.consistent_dE)
        v.why = "row-shared windows (grid): J must be symmetric with a zero diagonal";
    else if (!c.span.any)
        v.why = "row-shared windows (grid): J is all zero";
    else if (k > RS_GRID_MAX_K)
        v.why = "row-shared windows (grid): the couplings need a grid finer than 2^-30";
    else if (!(scaled <= 255.0))
        v.why = "row-shared windows (grid): 2^k max |J_ij| exceeds 255 (bit-planes of |2^k J|)";
    else if (!(fx_bound(c.row_abs_max, k) < 16777216.0))
        v.why = "row-shared windows (grid): 2^k max_i (sum_j |J_ij| + |h_i|) is not below 2^24";
    else if (c.acc_canon)
        v.why = "row-shared windows (grid): the couplings need the canonical fp64 summation order";
    else
        v.k = k, v.planes = scaled <= 1.0 ? 1 : scaled <= 7.0 ? 3 : 8;
    return v;
}

TspClass classify_tsp(const BitSpan &span, bool integral, double worst_row, int n_cities) {
    TspClass t;
    t.exact32 = integral && worst_row < 16777216.0;
    t.tsp_exact = t.exact32 || fp64_exact_any_order(span, 4ll * n_cities);
    return t;
}

void groups_span_add(BitSpan &s, float coeff, long long members) {
    if (members >= 2) span_add(s, coeff);
}

// the fp32-exact class: every coefficient on one grid 2^-k (the finest any coefficient or remainder value
// needs), 2^k max_i sum_{g contains i} |c_g| (|g| - 1) < 2^24
GroupsClass classify_groups(const BitSpan &coeffs, int rest_exp_lo_word, double worst) {
    GroupsClass g;
    int k = coeffs.any ? -coeffs.lo : INT_MIN;
    if (rest_exp_lo_word) k = std::max(k, rest_exp_lo_word - 1024);
    g.k = k == INT_MIN ? 0 : k;
    g.exact = !(g.k > 126 || std::ldexp(worst, g.k) >= 16777216.0);
    return g;
}

}  // namespace sga_classify
