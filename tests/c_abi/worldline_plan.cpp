// worldline_plan.cpp -- the admission rule of sga_worldline_clusters (sga_quantum.h: worldline_check,
// worldline_max_sites, worldline_lds_bytes, worldline_threshold), pure host arithmetic: no device call.
//   worldline_plan sites P...          the LDS budget, then per P: word bytes, the largest n served, the LDS bytes at that n
//   worldline_plan thr p...            the threshold of each bond probability
//   worldline_plan check have_engine have_p n R_local replica0 sstride csr tsp groups ragged n_models csr_acc metropolis
//                        consistent_dE n_sweeps n_slices p...
//                                      "ok", "invalid: <why>" or "unsupported: <why>"; p: the values of p_bond, the last
//                                      one repeated to n_sweeps * (R_local / n_slices) entries ("nan", "inf" read as such)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sga_quantum.h"

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "sites")) {
        std::printf("budget=%zu\n", sga::TRANSVERSE_LDS_BUDGET);
        for (int a = 2; a < argc; ++a) {
            const int P = std::atoi(argv[a]), n = sga::worldline_max_sites(P);
            std::printf("%d %d %zu\n", sga::worldline_word_bytes(P), n, sga::worldline_lds_bytes(n, P));
        }
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "thr")) {
        for (int a = 2; a < argc; ++a) std::printf("%u\n", sga::worldline_threshold(std::strtod(argv[a], nullptr)));
        return 0;
    }
    if (argc >= 18 && !std::strcmp(argv[1], "check")) {
        auto I = [&](int i) { return std::atoi(argv[i]); };
        sga::TrotterProblem p;
        p.n = I(4), p.R_local = I(5), p.replica0 = I(6), p.sstride = I(7);
        p.csr = I(8), p.tsp = I(9), p.groups = I(10), p.ragged = I(11), p.n_models = I(12);
        p.csr_acc = I(13), p.metropolis = I(14), p.consistent_dE = I(15);
        const int n_sweeps = I(16), n_slices = I(17);
        std::vector<double> b;
        for (int a = 18; a < argc; ++a) b.push_back(std::strtod(argv[a], nullptr));
        long long count = 1;
        if (n_sweeps > 0 && n_slices > 0 && p.R_local >= n_slices) count = (long long)n_sweeps * (p.R_local / n_slices);
        while ((long long)b.size() < count) b.push_back(b.empty() ? 0.0 : b.back());
        bool invalid = true;
        const char *why = sga::worldline_check(I(2) != 0, p, n_sweeps, n_slices, I(3) ? b.data() : nullptr, &invalid);
        std::printf("%s%s\n", !why ? "ok" : invalid ? "invalid: " : "unsupported: ", why ? why : "");
        return 0;
    }
    return 2;
}
