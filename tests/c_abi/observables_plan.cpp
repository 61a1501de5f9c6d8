// observables_plan.cpp -- the launch geometry of the replica observables' product (sga_kernels.h: observables_plan),
// pure host arithmetic: no device call.  Arguments: any number of queries, four integers each -- n, rows_a, rows_b,
// cus; each prints the tiles over the rows of A and of B, the K ranges and the columns per range.
#include <cstdio>
#include <cstdlib>

#include "sga_replicas.h"

int main(int argc, char **argv) {
    std::printf("tile=%d grain=%d kmin=%d\n", sga::OBS_TILE, sga::OBS_K_GRAIN, sga::OBS_K_MIN);
    for (int a = 1; a + 4 <= argc; a += 4) {
        const sga::ObservablesPlan p =
            sga::observables_plan(std::atoi(argv[a]), std::atoi(argv[a + 1]), std::atoi(argv[a + 2]), std::atoi(argv[a + 3]));
        std::printf("tiles_m=%d tiles_n=%d ksplit=%d kchunk=%d\n", p.tiles_m, p.tiles_n, p.ksplit, p.kchunk);
    }
    return 0;
}
