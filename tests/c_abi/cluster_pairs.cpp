// cluster_pairs.cpp -- the host half of the isoenergetic cluster moves (sga_kernels.h: cluster_lds_bytes,
// cluster_pairs_check), pure host arithmetic: no device call.
//   cluster_pairs lds n...                          budget and largest n, then the LDS bytes of every n
//   cluster_pairs check R replica0 reps a b a b...  "ok", or what sga_cluster_move_pairs says of the pair list
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sga_replicas.h"

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "lds")) {
        std::printf("budget=%zu max_n=%lld threads=%d\n", sga::CLUSTER_LDS_BUDGET, sga::CLUSTER_MAX_N, sga::CLUSTER_THREADS);
        for (int a = 2; a < argc; ++a) std::printf("%zu\n", sga::cluster_lds_bytes(std::atoll(argv[a])));
        return 0;
    }
    if (argc >= 5 && !std::strcmp(argv[1], "check") && (argc - 5) % 2 == 0) {
        const int R = std::atoi(argv[2]), replica0 = std::atoi(argv[3]), reps = std::atoi(argv[4]);
        std::vector<int32_t> pairs;
        for (int a = 5; a < argc; ++a) pairs.push_back((int32_t)std::atoi(argv[a]));
        std::vector<unsigned char> seen((size_t)(R > 0 ? R : 0));
        const char *why = sga::cluster_pairs_check(pairs.data(), (int)pairs.size() / 2, R, replica0, reps, seen.data());
        std::printf("%s\n", why ? why : "ok");
        return 0;
    }
    return 2;
}
