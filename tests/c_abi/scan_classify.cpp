// scan_classify.cpp -- the class sga_classify gives for scan words handed over as arguments (sga_get_scan_summary's words,
// or tests/scan_reference.py's), pure host code: no device call.  One line per case, default options, storage AUTO:
//   dense n n_models w0 .. w7                 -> the fields sga_get_route_query carries for a dense problem
//   csr n w0 .. w10                           -> ... for a CSR problem (w10: the longest row)
//   ragged M, then M times: n w0 .. w10       -> the batch-wide fold of the per-model classes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sga_classify.h"

using namespace sga_classify;

namespace {
CsrClass csr_of(char **w) {  // n, then the eleven words
    CsrScan s;
    const int n = std::atoi(w[0]);
    int f[11];
    for (int i = 0; i < 11; ++i) f[i] = std::atoi(w[1 + i]);
    s.not_integral = f[2];
    s.unsorted = f[3] != 0;
    s.diagonal = f[4] != 0;
    s.asymmetric = f[5] != 0;
    std::memcpy(&s.row_abs_max, &f[6], sizeof(float));
    s.exp_hi_word = f[7];
    s.exp_lo_word = f[8];
    std::memcpy(&s.row_j_abs_max, &f[9], sizeof(float));
    return classify_csr(s, f[10], n, {true, 0});
}
}  // namespace

int main(int argc, char **argv) {
    int a = 1;
    while (a < argc) {
        if (!std::strcmp(argv[a], "dense") && a + 11 <= argc) {
            int h[8];
            const int n = std::atoi(argv[a + 1]), M = std::atoi(argv[a + 2]);
            for (int i = 0; i < 8; ++i) h[i] = std::atoi(argv[a + 3 + i]);
            const DenseClass c = classify_dense(h, n, M, SGA_J_AUTO, false);
            std::printf("dense storage=%d acc=%d table_m=%d clf=%d bits=%d scale=%d dE=%d\n",
                        c.use_t2 ? SGA_J_T2 : (c.want_i8 ? SGA_J_I8 : SGA_J_F32), c.acc64 ? (c.acc_canon ? 2 : 1) : 0, c.table_m,
                        (int)c.clf_problem, c.clf_bits, c.clf_scale, (int)c.consistent_dE);
            a += 11;
        } else if (!std::strcmp(argv[a], "csr") && a + 13 <= argc) {
            const CsrClass c = csr_of(argv + a + 1);
            std::printf("csr acc=%d table_m=%d scale=%d clf=%d dE=%d sorted=%d\n", c.acc, c.table_m, c.table_scale, (int)c.clf_int16,
                        (int)c.consistent_dE, (int)c.sorted);
            a += 13;
        } else if (!std::strcmp(argv[a], "ragged") && a + 2 <= argc && a + 2 + 12 * std::atoi(argv[a + 1]) <= argc) {
            const int M = std::atoi(argv[a + 1]);
            std::vector<CsrClass> models;
            for (int m = 0; m < M; ++m) models.push_back(csr_of(argv + a + 2 + 12 * m));
            const RaggedClass b = fold_ragged(models, {0, false, false});
            std::printf("ragged acc=%d table_m=%d scale=%d sorted=%d\n", b.acc, b.table_m, b.table_scale, (int)b.sorted);
            a += 2 + 12 * M;
        } else {
            std::fprintf(stderr, "scan_classify: bad arguments at %d\n", a);
            return 2;
        }
    }
    return 0;
}
