// resample_check.cpp -- the host half of sga_resample (sga_kernels.h: resample_check, resample_scratch), pure host
// arithmetic: no device call.
//   resample_check check P R Rg replica0 n_models dbeta...  "ok", or what sga_resample says of the arguments
//   resample_check scratch R P                               the plan's scratch: offsets and bytes
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sga_replicas.h"

int main(int argc, char **argv) {
    if (argc >= 7 && !std::strcmp(argv[1], "check")) {
        const int P = std::atoi(argv[2]), R = std::atoi(argv[3]), Rg = std::atoi(argv[4]), replica0 = std::atoi(argv[5]),
                  n_models = std::atoi(argv[6]);
        std::vector<double> dbeta;
        for (int a = 7; a < argc; ++a) dbeta.push_back(std::strtod(argv[a], nullptr));  // ("nan", "inf" parse as such)
        // (one value given: every population's)
        if (dbeta.size() == 1 && P > 1) dbeta.resize((size_t)P, dbeta[0]);
        const char *why = sga::resample_check(P, dbeta.empty() ? nullptr : dbeta.data(), R, Rg, replica0, n_models);
        std::printf("%s\n", why ? why : "ok");
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "scratch")) {
        const sga::ResampleScratch s = sga::resample_scratch(std::atoll(argv[2]), std::atoll(argv[3]));
        std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", s.c, s.f, s.sp, s.parent, s.take, s.shift, s.sum, s.dbeta, s.bytes);
        std::printf("threads=%d max_members=%d copy_bytes=%d\n", sga::RESAMPLE_THREADS, sga::RESAMPLE_MAX_MEMBERS, sga::RESAMPLE_COPY_BYTES);
        return 0;
    }
    return 2;
}
