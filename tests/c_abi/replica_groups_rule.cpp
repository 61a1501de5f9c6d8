// replica_groups_rule.cpp -- the replica groups of the row-shared sweep (sga_kernels.h: row_shared_groups,
// row_shared_group_view, row_shared_groups_fit, row_shared_default_groups), pure host arithmetic: no device call.
// Arguments: any number of queries, five integers each -- n, W, S, R, G asked for.  Each prints one line: the groups the
// rule gives, whether their carve of the plan's scratch fits, the default count for R, and per group its range, where its
// views of cnt / ent / base / bits start (in elements), its plan groups, and its tile plan (replicas per slice, tiles per
// pass).
#include <cstdio>
#include <cstdlib>

#include "sga_kernels.h"

int main(int argc, char **argv) {
    std::printf("max=%d min_replicas=%d default_max=%d\n", sga::RS_MAX_GROUPS, sga::RS_GROUP_MIN_REPLICAS, sga::RS_DEFAULT_MAX_GROUPS);
    for (int a = 1; a + 5 <= argc; a += 5) {
        const int n = std::atoi(argv[a]), W = std::atoi(argv[a + 1]), S = std::atoi(argv[a + 2]), R = std::atoi(argv[a + 3]);
        const sga::RowSharedGroups g = sga::row_shared_groups(R, std::atoi(argv[a + 4]));
        std::printf("G=%d fit=%d default=%d", g.G, (int)sga::row_shared_groups_fit(n, W, S, R, g), sga::row_shared_default_groups(R));
        for (int i = 0; i < g.G; ++i) {
            const sga::RowSharedGroupView v = sga::row_shared_group_view(n, W, g, i);
            const sga::RowSharedTilePlan t = sga::row_shared_tile_plan(n, W, S, g.begin[i + 1] - g.begin[i]);
            std::printf(" | %d %d %lld %lld %lld %lld %d %d %d", g.begin[i], g.begin[i + 1], v.cnt, v.ent, v.base, v.bits, v.n_groups, t.rg,
                        t.tiles);
        }
        std::printf("\n");
    }
    return 0;
}
