// ladder_pairs_rule.cpp -- the preamble of the three calls that pair ladders slot by slot (sga_replicas.h:
// ladder_pairs_check), pure host code: no GPU, no library.
//   ladder_pairs_rule n_ladders have_slot_map R Rg slot_lo slot_hi noun...  ->  "ok L" | "refused L: text"
#include <cstdio>
#include <cstdlib>
#include <string>

#include "sga_replicas.h"

int main(int argc, char **argv) {
    if (argc < 8) return 2;
    std::string noun = argv[7];
    for (int i = 8; i < argc; ++i) noun += std::string(" ") + argv[i];
    const sga::LadderPairs lp = sga::ladder_pairs_check(std::atoi(argv[1]), std::atoi(argv[2]) != 0, std::atoi(argv[3]), std::atoi(argv[4]),
                                                        std::atoi(argv[5]), std::atoi(argv[6]), noun.c_str());
    if (lp.why)
        std::printf("refused %d: %s\n", lp.L, lp.why);
    else
        std::printf("ok %d\n", lp.L);
    return 0;
}
