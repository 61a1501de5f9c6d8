// worldline_dense_plan.cpp -- the admission rule of sga_worldline_clusters_dense (sga_quantum.h: worldline_dense_check),
// pure host arithmetic: no device call.
//   worldline_dense_plan check have_engine have_p n R_local replica0 sstride csr tsp groups ragged n_models clf_problem
//                              have_why field_bits ldf metropolis n_sweeps n_slices p...
//                                      "ok", "invalid: <why>" or "unsupported: <why>"; p: the values of p_bond, the last
//                                      one repeated to n_sweeps * (R_local / n_slices) entries ("nan", "inf" read as such)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sga_quantum.h"

int main(int argc, char **argv) {
    if (argc >= 20 && !std::strcmp(argv[1], "check")) {
        auto I = [&](int i) { return std::atoi(argv[i]); };
        sga::TrotterProblem p;
        p.n = I(4), p.R_local = I(5), p.replica0 = I(6), p.sstride = I(7);
        p.csr = I(8), p.tsp = I(9), p.groups = I(10), p.ragged = I(11), p.n_models = I(12);
        p.clf_problem = I(13), p.clf_why = I(14) ? "WHY FROM THE SCAN" : nullptr;
        p.field_bits = I(15), p.ldf = std::atoll(argv[16]), p.metropolis = I(17);
        const int n_sweeps = I(18), n_slices = I(19);
        std::vector<double> b;
        for (int a = 20; a < argc; ++a) b.push_back(std::strtod(argv[a], nullptr));
        long long count = 1;
        if (n_sweeps > 0 && n_slices > 0 && p.R_local >= n_slices) count = (long long)n_sweeps * (p.R_local / n_slices);
        while ((long long)b.size() < count) b.push_back(b.empty() ? 0.0 : b.back());
        bool invalid = true;
        const char *why = sga::worldline_dense_check(I(2) != 0, p, n_sweeps, n_slices, I(3) ? b.data() : nullptr, &invalid);
        std::printf("%s%s\n", !why ? "ok" : invalid ? "invalid: " : "unsupported: ", why ? why : "");
        return 0;
    }
    return 2;
}
