// trotter_exchange_plan.cpp -- the admission rules of sga_get_time_links and sga_exchange_transverse (sga_quantum.h:
// time_links_check, exchange_check), pure host arithmetic: no device call.
//   trotter_exchange_plan links    have_engine have_links n R_local replica0 csr tsp groups ragged n_models clf_problem
//                                  metropolis n_slices
//   trotter_exchange_plan exchange have_engine have_k n R_local replica0 csr tsp groups ragged n_models clf_problem
//                                  metropolis n_slices R_global parity k...
//                                      "ok", "invalid: <why>" or "unsupported: <why>"; k: the values of k_perp, the last
//                                      one repeated to R_local / n_slices entries ("nan", "inf" read as such)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sga_quantum.h"

int main(int argc, char **argv) {
    if (argc < 15) return 2;
    auto I = [&](int i) { return std::atoi(argv[i]); };
    sga::TrotterProblem p;
    p.n = I(4), p.R_local = I(5), p.replica0 = I(6), p.sstride = (I(4) + 15) / 16 * 16;
    p.csr = I(7), p.tsp = I(8), p.groups = I(9), p.ragged = I(10), p.n_models = I(11);
    p.clf_problem = I(12), p.metropolis = I(13);
    const int n_slices = I(14);
    bool invalid = true;
    const char *why = nullptr;
    if (!std::strcmp(argv[1], "links") && argc == 15) {
        int64_t one = 0;
        why = sga::time_links_check(I(2) != 0, p, n_slices, I(3) ? &one : nullptr, &invalid);  // (nothing of links is read)
    } else if (!std::strcmp(argv[1], "exchange") && argc >= 17) {
        p.R_global = I(15);
        std::vector<float> k;
        for (int a = 17; a < argc; ++a) k.push_back(std::strtof(argv[a], nullptr));
        long long count = 1;
        if (n_slices > 0 && p.R_local >= n_slices) count = p.R_local / n_slices;
        while ((long long)k.size() < count) k.push_back(k.empty() ? 0.0f : k.back());
        why = sga::exchange_check(I(2) != 0, p, n_slices, I(3) ? k.data() : nullptr, I(16), &invalid);
    } else {
        return 2;
    }
    std::printf("%s%s\n", !why ? "ok" : invalid ? "invalid: " : "unsupported: ", why ? why : "");
    return 0;
}
