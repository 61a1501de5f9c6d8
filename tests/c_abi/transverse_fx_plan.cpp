// transverse_fx_plan.cpp -- the admission rule of sga_sweep_transverse_dense on fixed-point fields (sga_quantum.h:
// transverse_dense_check with TrotterProblem::fx_bits / fx_why, transverse_dense_lds_bytes) and worldline_dense_check's
// answer to such a problem; pure host arithmetic: no device call.
//   transverse_fx_plan lds ldf fbytes sstride     the LDS budget, then the bytes a slice of that shape takes
//   transverse_fx_plan check key=value ...        transverse_dense_check: "ok", "invalid: <why>" or "unsupported: <why>"
//   transverse_fx_plan worldline key=value ...    worldline_dense_check, likewise (p_bond = 0.5 throughout)
// keys: have_engine have_k n R_local replica0 sstride csr tsp groups ragged n_models clf_problem have_why field_bits ldf
// fx_bits have_fx_why metropolis n_sweeps n_slices arith_ok k (one value of k_perp for every entry; "nan", "inf" read as
// such).  have_why: the integer scan left "WHY FROM THE SCAN"; have_fx_why: the fixed-point verdict left "WHY FROM THE FX
// VERDICT".  A key not given keeps the value of a served int32 problem.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "sga_quantum.h"

int main(int argc, char **argv) {
    if (argc == 5 && !std::strcmp(argv[1], "lds")) {
        std::printf("budget=%zu\n%zu\n", sga::TRANSVERSE_LDS_BUDGET,
                    sga::transverse_dense_lds_bytes(std::atoll(argv[2]), std::atoi(argv[3]), std::atoi(argv[4])));
        return 0;
    }
    if (argc < 2 || (std::strcmp(argv[1], "check") && std::strcmp(argv[1], "worldline"))) return 2;
    std::map<std::string, std::string> kv = {{"have_engine", "1"}, {"have_k", "1"}, {"n", "100"}, {"R_local", "12"}, {"replica0", "0"},
                                             {"sstride", "128"}, {"csr", "0"}, {"tsp", "0"}, {"groups", "0"}, {"ragged", "0"},
                                             {"n_models", "1"}, {"clf_problem", "0"}, {"have_why", "1"}, {"field_bits", "16"},
                                             {"ldf", "128"}, {"fx_bits", "32"}, {"have_fx_why", "0"}, {"metropolis", "1"},
                                             {"n_sweeps", "3"}, {"n_slices", "4"}, {"arith_ok", "1"}, {"k", "0.25"}};
    for (int a = 2; a < argc; ++a) {
        const char *eq = std::strchr(argv[a], '=');
        if (!eq) return 2;
        const std::string key(argv[a], (size_t)(eq - argv[a]));
        if (!kv.count(key)) return 2;
        kv[key] = eq + 1;
    }
    auto I = [&](const char *key) { return std::atoi(kv[key].c_str()); };
    sga::TrotterProblem p;
    p.n = I("n"), p.R_local = I("R_local"), p.replica0 = I("replica0"), p.sstride = I("sstride");
    p.csr = I("csr"), p.tsp = I("tsp"), p.groups = I("groups"), p.ragged = I("ragged"), p.n_models = I("n_models");
    p.clf_problem = I("clf_problem");
    p.clf_why = I("have_why") ? "WHY FROM THE SCAN" : nullptr;
    p.field_bits = I("field_bits"), p.ldf = std::atoll(kv["ldf"].c_str()), p.metropolis = I("metropolis");
    p.fx_bits = I("fx_bits");
    p.fx_why = I("have_fx_why") ? "WHY FROM THE FX VERDICT" : nullptr;
    const int n_sweeps = I("n_sweeps"), n_slices = I("n_slices");
    long long count = 1;
    if (n_sweeps > 0 && n_slices > 0 && p.R_local >= n_slices) count = (long long)n_sweeps * (p.R_local / n_slices);
    bool invalid = true;
    const char *why = nullptr;
    if (!std::strcmp(argv[1], "check")) {
        const std::vector<float> k((size_t)count, std::strtof(kv["k"].c_str(), nullptr));
        why = sga::transverse_dense_check(I("have_engine") != 0, p, n_sweeps, n_slices, I("arith_ok") != 0, I("have_k") ? k.data() : nullptr, &invalid);
    } else {
        const std::vector<double> b((size_t)count, 0.5);
        why = sga::worldline_dense_check(I("have_engine") != 0, p, n_sweeps, n_slices, I("have_k") ? b.data() : nullptr, &invalid);
    }
    std::printf("%s%s\n", !why ? "ok" : invalid ? "invalid: " : "unsupported: ", why ? why : "");
    return 0;
}
