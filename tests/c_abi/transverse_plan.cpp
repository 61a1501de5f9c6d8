// transverse_plan.cpp -- the admission rule of sga_sweep_transverse (sga_quantum.h: transverse_check,
// transverse_waves_per_block), pure host arithmetic: no device call.
//   transverse_plan waves sstride...   the LDS budget, then the waves per workgroup of each spin stride
//   transverse_plan slices P parity    the slice geometry of a half-sweep (moving_slice): per moving index m of three groups
//                                      of P slices, "g r up dn" -- its group, its row and its two neighbours' rows
//   transverse_plan check have_engine have_k n R_local replica0 sstride csr tsp groups ragged n_models csr_acc metropolis
//                         consistent_dE n_sweeps n_slices arith_ok k...
//                                      "ok", "invalid: <why>" or "unsupported: <why>"; k: the values of k_perp, the last
//                                      one repeated to n_sweeps * (R_local / n_slices) entries ("nan", "inf", "-inf" read
//                                      as such)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sga_quantum.h"

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "waves")) {
        std::printf("budget=%zu\n", sga::TRANSVERSE_LDS_BUDGET);
        for (int a = 2; a < argc; ++a) std::printf("%d\n", sga::transverse_waves_per_block(std::atoi(argv[a])));
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "slices")) {
        const int P = std::atoi(argv[2]), parity = std::atoi(argv[3]);
        for (int m = 0; m < 3 * (P / 2); ++m) {  // three groups
            const sga::MovingSlice s = sga::moving_slice(m, P, parity);
            std::printf("%d %d %d %d\n", s.g, s.r, s.up, s.dn);
        }
        return 0;
    }
    if (argc >= 20 && !std::strcmp(argv[1], "check")) {
        auto I = [&](int i) { return std::atoi(argv[i]); };
        sga::TrotterProblem p;
        p.n = I(4), p.R_local = I(5), p.replica0 = I(6), p.sstride = I(7);
        p.csr = I(8), p.tsp = I(9), p.groups = I(10), p.ragged = I(11), p.n_models = I(12);
        p.csr_acc = I(13), p.metropolis = I(14), p.consistent_dE = I(15);
        const int n_sweeps = I(16), n_slices = I(17);
        std::vector<float> k;
        for (int a = 19; a < argc; ++a) k.push_back(std::strtof(argv[a], nullptr));
        long long count = 1;
        if (n_sweeps > 0 && n_slices > 0 && p.R_local >= n_slices) count = (long long)n_sweeps * (p.R_local / n_slices);
        while ((long long)k.size() < count) k.push_back(k.empty() ? 0.0f : k.back());
        bool invalid = true;
        const char *why = sga::transverse_check(I(2) != 0, p, n_sweeps, n_slices, I(18) != 0, I(3) ? k.data() : nullptr, &invalid);
        std::printf("%s%s\n", !why ? "ok" : invalid ? "invalid: " : "unsupported: ", why ? why : "");
        return 0;
    }
    return 2;
}
