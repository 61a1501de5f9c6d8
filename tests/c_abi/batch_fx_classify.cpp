// batch_fx_classify.cpp -- the fixed-point verdict over many-model dense batches (sga_classify::dense_fixed_point with
// batch_allowed, option "batch_fixed_point"), pure host code: no device call.  Arguments: any number of stacked scans,
// ten integers each -- n, n_models and the eight scan words classify_dense reads (tests/batch_fx_cases.py, scan_words);
// each prints its batch verdict.  Then the refusals over a batch and the calls without the new argument.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sga_classify.h"

using namespace sga_classify;

namespace {
int bits_of(float v) {
    int b;
    std::memcpy(&b, &v, sizeof(b));
    return b;
}
void fx(const char *name, const FxVerdict &v) { std::printf("%s: bits=%d k=%d why=%s\n", name, v.bits, v.k, v.why ? v.why : "-"); }
}  // namespace

int main(int argc, char **argv) {
    int asked = 0;
    const auto yes = [&] { return ++asked, true; };
    const auto no = [&] { return ++asked, false; };
    std::printf("# cases\n");
    for (int a = 1; a + 10 <= argc; a += 10) {
        int h[8];
        const int n = std::atoi(argv[a]), M = std::atoi(argv[a + 1]);
        for (int i = 0; i < 8; ++i) h[i] = std::atoi(argv[a + 2 + i]);
        const DenseClass c = classify_dense(h, n, M, SGA_J_AUTO, false);
        char name[64];
        std::snprintf(name, sizeof(name), "case %d clf=%d i8=%d", (a - 1) / 10, (int)c.clf_problem, (int)c.want_i8);
        fx(name, dense_fixed_point(c, M, yes, true));
    }
    std::printf("asked=%d\n", asked);
    std::printf("# thresholds\n");
    {
        // not int8, not ternary, real-valued J, symmetric: the stacked maximum decides the width, the stacked span decides k
        int h[8] = {1, 1, bits_of(2047.0f), 1, 0, 1024 - 10, 1024 + 20, bits_of(1.0f)};
        fx("2047 k 20", dense_fixed_point(classify_dense(h, 64, 3, SGA_J_AUTO, false), 3, yes, true));
        h[2] = bits_of(2048.0f);
        fx("2048 k 20", dense_fixed_point(classify_dense(h, 64, 3, SGA_J_AUTO, false), 3, yes, true));
        h[2] = bits_of(33554432.0f), h[3] = 4, h[5] = 1024 + 20, h[6] = 1024 - 2;  // integer J, h off the half-integers
        fx("k clamped", dense_fixed_point(classify_dense(h, 64, 3, SGA_J_AUTO, false), 3, yes, true));
    }
    std::printf("# refusals\n");
    {
        asked = 0;
        int h[8] = {1, 1, bits_of(1048576.0f), 1, 1, 1024 - 40, 1024 + 42, bits_of(1.0f)};  // 2^20 2^42: wider than int64
        fx("all", dense_fixed_point(classify_dense(h, 64, 3, SGA_J_AUTO, true), 3, yes, true));  // (canonical forced)
        std::printf("asked=%d\n", asked);
        fx("diagonal", dense_fixed_point(classify_dense(h, 64, 3, SGA_J_AUTO, false), 3, yes, true));
        fx("asymmetric", dense_fixed_point(classify_dense(h, 64, 3, SGA_J_AUTO, false), 3, no, true));
        h[4] = 0;
        fx("width", dense_fixed_point(classify_dense(h, 64, 3, SGA_J_AUTO, false), 3, yes, true));
        std::printf("asked=%d\n", asked);
        h[5] = 1024 + 2, h[6] = 1024 + 60, h[2] = bits_of(200.0f);  // O(1) couplings beside one of 2^-60: span 63 bits
        fx("span", dense_fixed_point(classify_dense(h, 200, 3, SGA_J_AUTO, false), 3, yes, true));
    }
    std::printf("# without the option\n");
    {
        int h[8] = {1, 1, bits_of(2047.0f), 1, 0, 1024 - 10, 1024 + 20, bits_of(1.0f)};
        const DenseClass c3 = classify_dense(h, 64, 3, SGA_J_AUTO, false), c1 = classify_dense(h, 64, 1, SGA_J_AUTO, false);
        fx("three arguments, batch", dense_fixed_point(c3, 3, yes));
        fx("batch_allowed = false, batch", dense_fixed_point(c3, 3, yes, false));
        fx("three arguments, one model", dense_fixed_point(c1, 1, yes));
        fx("batch_allowed = true, one model", dense_fixed_point(c1, 1, yes, true));
    }
    return 0;
}
