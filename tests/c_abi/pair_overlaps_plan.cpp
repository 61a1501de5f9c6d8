// pair_overlaps_plan.cpp -- the host half of the pair overlaps (sga_kernels.h: pair_overlap_lds_bytes,
// pair_overlap_group_log2, pair_overlap_pairs_check, pair_overlap_hist_check), pure host arithmetic: no device call.
//   pair_overlaps_plan lds n...                 budget, largest n and threads, then "<bytes with links> <bytes without>" per n
//   pair_overlaps_plan group entries n          lanes to a row, as log2
//   pair_overlaps_plan pairs R count a b a b... "ok", or what sga_get_pair_overlaps says of the pair list ("null": no list)
//   pair_overlaps_plan hist have_q bins_q q_shift have_l bins_l l_shift
//                                               "ok", or what sga_accumulate_ladder_overlaps says of the histogram arguments
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sga_replicas.h"

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "lds")) {
        std::printf("budget=%zu max_n=%lld threads=%d\n", sga::CLUSTER_LDS_BUDGET, sga::PAIR_OVERLAP_MAX_N, sga::PAIR_OVERLAP_THREADS);
        for (int a = 2; a < argc; ++a)
            std::printf("%zu %zu\n", sga::pair_overlap_lds_bytes(std::atoll(argv[a]), true),
                        sga::pair_overlap_lds_bytes(std::atoll(argv[a]), false));
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "group")) {
        std::printf("%d\n", sga::pair_overlap_group_log2(std::atoll(argv[2]), std::atoll(argv[3])));
        return 0;
    }
    if (argc >= 4 && !std::strcmp(argv[1], "pairs")) {
        const int R = std::atoi(argv[2]), count = std::atoi(argv[3]);
        std::vector<int32_t> pairs;
        const bool null_list = argc == 5 && !std::strcmp(argv[4], "null");
        for (int a = 4; a < argc && !null_list; ++a) pairs.push_back((int32_t)std::atoi(argv[a]));
        if (!null_list && count > 0 && (int)pairs.size() != 2 * count) return 2;
        const char *why = sga::pair_overlap_pairs_check(null_list ? nullptr : pairs.data(), count, R);
        std::printf("%s\n", why ? why : "ok");
        return 0;
    }
    if (argc == 8 && !std::strcmp(argv[1], "hist")) {
        const char *why = sga::pair_overlap_hist_check(std::atoi(argv[2]) != 0, std::atoi(argv[3]), std::atoi(argv[4]),
                                                       std::atoi(argv[5]) != 0, std::atoi(argv[6]), std::atoi(argv[7]));
        std::printf("%s\n", why ? why : "ok");
        return 0;
    }
    return 2;
}
