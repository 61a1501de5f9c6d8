// rs_accept_table_rule.cpp -- the size of the chain's accept table (sga_kernels.h: rs_accept_table_entries,
// rs_accept_table_zero_from), pure host arithmetic: no device call.  Arguments: any number of queries, two words each --
// T (anything strtod reads: hexadecimal floats, inf) and table_m; each prints the entries Q and the q from which every
// probability is zero (2147483647: no such bound).
#include <cstdio>
#include <cstdlib>

#include "sga_kernels.h"

int main(int argc, char **argv) {
    std::printf("max=%d\n", sga::RS_ACCEPT_TABLE_MAX);
    for (int a = 1; a + 2 <= argc; a += 2) {
        const double T = std::strtod(argv[a], nullptr);
        const int table_m = std::atoi(argv[a + 1]);
        std::printf("Q=%d zero_from=%d\n", sga::rs_accept_table_entries(T, table_m), sga::rs_accept_table_zero_from(T));
    }
    return 0;
}
