// rs_grid_classify.cpp -- the grid verdict of the row-shared windows (sga_classify::row_shared_grid, option
// "row_shared_grid"), pure host code: no device call.  Arguments: any number of scans, ten integers each -- n, the
// storage selector and the eight scan words classify_dense reads (tests/scan_reference.py, dense_words); each prints the
// class the verdict starts from and the verdict.
#include <cstdio>
#include <cstdlib>

#include "sga_classify.h"

using namespace sga_classify;

int main(int argc, char **argv) {
    for (int a = 1; a + 10 <= argc; a += 10) {
        int h[8];
        const int n = std::atoi(argv[a]), storage = std::atoi(argv[a + 1]);
        for (int i = 0; i < 8; ++i) h[i] = std::atoi(argv[a + 2 + i]);
        const DenseClass c = classify_dense(h, n, 1, storage, false);
        const RsGridVerdict v = row_shared_grid(c);
        std::printf("case %d table_m=%d acc64=%d canon=%d j_max=%.9g: k=%d planes=%d why=%s\n", (a - 1) / 10, c.table_m, (int)c.acc64,
                    (int)c.acc_canon, (double)c.j_max, v.k, v.planes, v.why ? v.why : "-");
    }
    return 0;
}
