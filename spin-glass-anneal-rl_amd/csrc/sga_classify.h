// sga_classify.h -- WHICH arithmetic a problem admits: pure functions of the set-time scan summaries (flag words, row
// maxima, longest row, options).  No device call and no sga_engine anywhere in sga_classify.cpp; the setters of
// sga_problem.cpp scan and copy, ask here once, and assign the engine's fields from the answer.  The other half of
// sga_route.h (which FORM then runs).
#ifndef SGA_CLASSIFY_H
#define SGA_CLASSIFY_H
#include <functional>
#include <string>
#include <vector>

#include "sga.h"

namespace sga_classify {

// ---- bit spans ------------------------------------------------------------------------------------------------------
// binary exponents of the highest and the lowest set bit over a set of fp32 values
struct BitSpan {
    int hi = -10000, lo = 10000;
    bool any = false;  // some non-zero value was seen
};
void span_add(BitSpan &s, float v);                  // zero and non-finite values are ignored
BitSpan span_of_words(int hi_word, int lo_word);     // from the scans' biased words: 1024 + hi, 1024 - lo (0, 0: no value)
int carry_bits(long long terms);                     // the smallest c with 2^c >= max(terms, 1)
bool fp64_exact_any_order(const BitSpan &s, long long terms);

// ---- cached local fields as exact fixed point (option "clf_fixed_point") ----------------------------------------------
constexpr double FX_LIMIT_ONE = 0x1.0p62;     // one problem (dense, CSR): fields up to int64 -- kept as found
constexpr double FX_LIMIT_RAGGED = 0x1.0p53;  // per model of a ragged batch: the fp64 seed sums stay exact -- kept as found
struct FxVerdict {
    int bits = 0, k = 0;        // 32 | 64 and the grid 2^-k where the form applies
    const char *why = nullptr;  // else the first condition that fails
};
struct FxQuery {
    BitSpan span;               // of J: k = minus the exponent of its lowest set bit
    bool clamp_k = false;       // k >= 0
    double field_max = 0.0;     // the maximum that bounds the fields
    bool batch = false, canonical = false, unsorted = false, consistent_dE = true, n_too_large = false;
    bool stacked = false;       // a dense batch scanned as a whole: the reasons name what SOME model does
};
double fx_bound(double field_max, int k);  // 2^k field_max, the fp32 rounding of field_max allowed for
inline int fx_bits(double bound) { return bound < 0x1.0p31 ? 32 : 64; }
// diagonal: asked only when consistent_dE is false and nothing earlier in the list failed
FxVerdict fixed_point_verdict(const FxQuery &q, const std::function<bool()> &diagonal);

// ---- CSR couplings ---------------------------------------------------------------------------------------------------
enum { ACC_F32_TABLE = 0, ACC_F32 = 1, ACC_F64 = 2, ACC_F64_CANON = 3 };  // == sga::CSR_ACC_* (sga_kernels.h)
struct CsrScan {  // the flag words of launch_csr_scan / launch_csr_symmetry (sga_kernels.h: CSR_*) by name
    int not_integral = 0;  // bit 0: some J, bit 1: some h not an integer, bit 2: some h not a multiple of 1/2
    bool unsorted = false, diagonal = false, asymmetric = false;
    float row_abs_max = 0.0f, row_j_abs_max = 0.0f;
    int exp_hi_word = 0, exp_lo_word = 0;
};
struct CsrOptions {
    bool half_integer_table = true;
    int force_csr_acc = 0;
};
struct CsrClass {
    int acc = ACC_F64_CANON, table_m = 0, table_scale = 1;
    bool consistent_dE = false, sorted = false, clf_int16 = false, x_exact = false;
    float row_abs_max = 0.0f, row_j_abs_max = 0.0f;
    CsrScan scan;  // as handed in (the fixed-point verdict and the ragged fold read it)
    BitSpan span;
    long long longest_row = 0;
};
CsrClass classify_csr(const CsrScan &s, long long longest_row, int n, const CsrOptions &o);
FxVerdict csr_fixed_point(const CsrClass &c, int n);

// ragged batches (sga_set_csr_batch): the per-model classes (classify_csr with force_csr_acc = 0) folded batch-wide
struct RaggedOptions {
    int force_csr_acc = 0;
    bool want_clf = false, want_fx = false;  // options "ragged_field_cache", and "clf_fixed_point" with it
};
struct RaggedClass {
    int acc = ACC_F32_TABLE, table_m = 0, table_scale = 1;
    bool sorted = true, clf_problem = false;
    float row_abs_max = 0.0f, row_j_abs_max = 0.0f;
    std::string clf_why;  // the first model that keeps the batch off the cached-field forms and why (empty: none, or not asked)
    int fx_bits = 0, fx_k = 0;
};
RaggedClass fold_ragged(const std::vector<CsrClass> &models, const RaggedOptions &o);

// ---- dense couplings ---------------------------------------------------------------------------------------------------
struct DenseClass {
    bool consistent_dE = false, fits_i8 = false, ternary = false, use_t2 = false, want_i8 = false;
    bool acc64 = false, acc_canon = false, clf_problem = false;
    unsigned nonint = 0;  // bit 0: some J, bit 1: some h not an integer, bit 2: some h not a multiple of 1/2
    int table_m = 0, clf_scale = 1, clf_bits = 16, j_abs_max = 0;
    float row_abs_max = 0.0f;
    float j_max = 0.0f;   // max |J_ij| as the scan wrote it (word [7]; j_abs_max is its ceiling)
    BitSpan span;
};
// hflags: the eight words of launch_scan_values / launch_dense_row_abs_max / launch_check_symmetric
DenseClass classify_dense(const int hflags[8], int n, int n_models, int storage, bool force_dense_canonical);
// a problem with !clf_problem: which condition of the integer cached-field form failed, and the fixed-point verdict
const char *dense_clf_why(const DenseClass &c, const std::function<bool()> &diagonal);
// batch_allowed (option "batch_fixed_point"): a many-model batch gets the one-model verdict over its stacked scan
FxVerdict dense_fixed_point(const DenseClass &c, int n_models, const std::function<bool()> &diagonal, bool batch_allowed = false);

// Row-shared windows on a binary grid (option "row_shared_grid", sweep_dense_rs.hip): the dense problems the integer
// form of the windows does not take -- J on a grid 2^-k whose scaled values 2^k J_ij are integers of at most 255, every
// scaled row sum below 2^24 -- under any finite fp32 h.  A shared-coupling batch hands in the batch's words.
constexpr int RS_GRID_MAX_K = 30;  // a declared limit (2^k is formed as an int and as a float)
struct RsGridVerdict {
    int k = 0, planes = 0;      // the grid 2^-k and the magnitude planes of |2^k J| (1 | 3 | 8) where the form applies
    const char *why = nullptr;  // else the first condition that fails
};
RsGridVerdict row_shared_grid(const DenseClass &c);

// ---- implicit couplings --------------------------------------------------------------------------------------------------
struct TspClass {
    bool exact32 = false, tsp_exact = false;
};
// span / integral: over the scaled distances and the two penalties; worst_row: max over sites of sum_j |J_ij|
TspClass classify_tsp(const BitSpan &span, bool integral, double worst_row, int n_cities);

struct GroupsClass {
    int k = 0;           // every coefficient and remainder value on the grid 2^-k
    bool exact = false;  // a combined row sum is exact in fp32 in any order
};
void groups_span_add(BitSpan &s, float coeff, long long members);  // (fewer than two members: contributes no coupling)
GroupsClass classify_groups(const BitSpan &coeffs, int rest_exp_lo_word, double worst);

}  // namespace sga_classify

#endif  // SGA_CLASSIFY_H
