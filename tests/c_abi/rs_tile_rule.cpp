// rs_tile_rule.cpp -- the tile size of the row-shared fields kernel (sga_kernels.h: row_shared_tile_sites,
// row_shared_tile_lds; option "row_shared_fields"), pure host arithmetic: no device call.  Arguments: any number of
// queries, six integers each -- n, planes, sign-only, R, CUs, forced S; each prints S, the kernel's LDS bytes at that S
// the reason where the per-site kernel runs, and whether option "row_shared_fields" = 2 takes the tiles (dflt=).
#include <cstdio>
#include <cstdlib>

#include "sga_kernels.h"

int main(int argc, char **argv) {
    std::printf("threads=%d entries=%d max_replicas=%d max_sites=%d budget=%zu\n", sga::RS_TILE_THREADS, sga::RS_TILE_ENTRIES,
                sga::RS_TILE_MAX_REPLICAS, sga::RS_TILE_MAX_SITES, sga::RS_TILE_LDS_BUDGET);
    for (int a = 1; a + 6 <= argc; a += 6) {
        const int n = std::atoi(argv[a]), planes = std::atoi(argv[a + 1]), ones = std::atoi(argv[a + 2]), R = std::atoi(argv[a + 3]),
                  cus = std::atoi(argv[a + 4]), forced = std::atoi(argv[a + 5]);
        const char *why = nullptr;
        const int S = sga::row_shared_tile_sites(n, planes, ones != 0, R, cus, forced, &why);
        std::printf("S=%d lds=%zu why=%s dflt=%d\n", S, S > 0 ? sga::row_shared_tile_lds(n, planes, ones != 0, S, R) : (size_t)0,
                    why ? why : "-", S > 0 && !sga::row_shared_tiles_not_default(n, planes, ones != 0));
    }
    return 0;
}
