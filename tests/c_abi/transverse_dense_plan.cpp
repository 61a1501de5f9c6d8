// transverse_dense_plan.cpp -- the admission rule of sga_sweep_transverse_dense (sga_quantum.h: transverse_dense_check,
// transverse_dense_lds_bytes), pure host arithmetic: no device call.
//   transverse_dense_plan lds ldf fbytes sstride      the LDS budget, then the bytes a slice of that shape takes
//   transverse_dense_plan check have_engine have_k n R_local replica0 sstride csr tsp groups ragged n_models clf_problem
//                               have_why field_bits ldf metropolis n_sweeps n_slices arith_ok k...
//                                      "ok", "invalid: <why>" or "unsupported: <why>"; have_why: the set-time scan left a
//                                      reason ("WHY FROM THE SCAN"); k: the values of k_perp, the last one repeated to
//                                      n_sweeps * (R_local / n_slices) entries ("nan", "inf", "-inf" read as such)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sga_quantum.h"

int main(int argc, char **argv) {
    if (argc == 5 && !std::strcmp(argv[1], "lds")) {
        std::printf("budget=%zu\n%zu\n", sga::TRANSVERSE_LDS_BUDGET,
                    sga::transverse_dense_lds_bytes(std::atoll(argv[2]), std::atoi(argv[3]), std::atoi(argv[4])));
        return 0;
    }
    if (argc >= 22 && !std::strcmp(argv[1], "check")) {
        auto I = [&](int i) { return std::atoi(argv[i]); };
        sga::TrotterProblem p;
        p.n = I(4), p.R_local = I(5), p.replica0 = I(6), p.sstride = I(7);
        p.csr = I(8), p.tsp = I(9), p.groups = I(10), p.ragged = I(11), p.n_models = I(12);
        p.clf_problem = I(13);
        p.clf_why = I(14) ? "WHY FROM THE SCAN" : nullptr;
        p.field_bits = I(15), p.ldf = std::atoll(argv[16]), p.metropolis = I(17);
        const int n_sweeps = I(18), n_slices = I(19);
        std::vector<float> k;
        for (int a = 21; a < argc; ++a) k.push_back(std::strtof(argv[a], nullptr));
        long long count = 1;
        if (n_sweeps > 0 && n_slices > 0 && p.R_local >= n_slices) count = (long long)n_sweeps * (p.R_local / n_slices);
        while ((long long)k.size() < count) k.push_back(k.empty() ? 0.0f : k.back());
        bool invalid = true;
        const char *why = sga::transverse_dense_check(I(2) != 0, p, n_sweeps, n_slices, I(20) != 0, I(3) ? k.data() : nullptr, &invalid);
        std::printf("%s%s\n", !why ? "ok" : invalid ? "invalid: " : "unsupported: ", why ? why : "");
        return 0;
    }
    return 2;
}
