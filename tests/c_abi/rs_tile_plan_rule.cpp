// rs_tile_plan_rule.cpp -- the geometry of the tile kernel's plan (sga_kernels.h: row_shared_tile_plan,
// row_shared_tile_plan_lds, row_shared_tile_plan_runs_fit), pure host arithmetic: no device call.  Arguments: any number
// of queries, four integers each -- n, W, S, R; each prints the replicas per slice, the tiles a workgroup covers in one
// pass, the LDS bytes the plan asks for and whether the run starts fit the by-site plan's counts.
#include <cstdio>
#include <cstdlib>

#include "sga_kernels.h"

int main(int argc, char **argv) {
    std::printf("threads=%d extra=%d lds=%zu budget=%zu\n", sga::RS_TILE_PLAN_THREADS, sga::RS_TILE_PLAN_EXTRA, sga::RS_TILE_PLAN_LDS,
                sga::RS_TILE_LDS_BUDGET);
    for (int a = 1; a + 4 <= argc; a += 4) {
        const int n = std::atoi(argv[a]), W = std::atoi(argv[a + 1]), S = std::atoi(argv[a + 2]), R = std::atoi(argv[a + 3]);
        const sga::RowSharedTilePlan t = sga::row_shared_tile_plan(n, W, S, R);
        std::printf("rg=%d tiles=%d lds=%zu fit=%d\n", t.rg, t.tiles, t.rg ? sga::row_shared_tile_plan_lds(W, t.rg, t.tiles) : (size_t)0,
                    t.rg ? (int)sga::row_shared_tile_plan_runs_fit(n, W, S, R, t.rg) : 0);
    }
    return 0;
}
