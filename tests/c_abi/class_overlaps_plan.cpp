// class_overlaps_plan.cpp -- the host half of the class-resolved overlaps (sga_kernels.h: class_overlap_copies,
// class_overlap_lds_bytes, CLASS_OVERLAP_MAX_MC, class_overlap_args_check, class_overlap_unsupported), pure host
// arithmetic: no device call.
//   class_overlaps_plan lds mc...    budget, the bound on n_maps * n_classes, the largest product with four copies and
//                                    threads, then "<copies> <LDS bytes>" per product
//   class_overlaps_plan args have_classes have_out n_maps n_classes ld n
//                                    "ok", "invalid: <why>" or "unsupported: <why>", in the order the calls check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sga_replicas.h"

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "lds")) {
        std::printf("budget=%zu max_mc=%lld max_mc_4=%lld threads=%d\n", sga::CLUSTER_LDS_BUDGET, sga::CLASS_OVERLAP_MAX_MC,
                    sga::CLASS_OVERLAP_MAX_MC_4, sga::CLASS_OVERLAP_THREADS);
        for (int a = 2; a < argc; ++a)
            std::printf("%d %zu\n", sga::class_overlap_copies(std::atoll(argv[a])), sga::class_overlap_lds_bytes(std::atoll(argv[a])));
        return 0;
    }
    if (argc == 8 && !std::strcmp(argv[1], "args")) {
        const int n_maps = std::atoi(argv[4]), n_classes = std::atoi(argv[5]);
        if (const char *why = sga::class_overlap_args_check(std::atoi(argv[2]) != 0, std::atoi(argv[3]) != 0, n_maps, n_classes,
                                                            std::atoll(argv[6]), std::atoll(argv[7]))) {
            std::printf("invalid: %s\n", why);
            return 0;
        }
        const char *why = sga::class_overlap_unsupported(n_maps, n_classes);
        std::printf("%s%s\n", why ? "unsupported: " : "ok", why ? why : "");
        return 0;
    }
    return 2;
}
