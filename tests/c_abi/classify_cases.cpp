// classify_cases.cpp -- drives the set-time classification (sga_classify.h) over scan summaries that sit on and beside
// every threshold and prints one line per case; tests/test_classify_host.py compares the print with lines written out
// by hand from the thresholds.  No device call: libsga.so is only linked for sga_classify.cpp.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "sga_classify.h"

using namespace sga_classify;

namespace {

// a CSR scan: integer / non-integer bits, max_i (sum |J| + |h|), max_i sum |J|, exponents of J's highest / lowest set bit
CsrScan scan(int not_integral, float m, float mj, int hi, int lo) {
    CsrScan s;
    s.not_integral = not_integral;
    s.row_abs_max = m;
    s.row_j_abs_max = mj;
    s.exp_hi_word = 1024 + hi;
    s.exp_lo_word = 1024 - lo;
    return s;
}
CsrClass csr(const char *name, const CsrScan &s, long long longest = 8, int n = 64, CsrOptions o = {true, 0}) {
    const CsrClass c = classify_csr(s, longest, n, o);
    std::printf("%s: acc=%d table_m=%d scale=%d dE=%d sorted=%d i16=%d x=%d\n", name, c.acc, c.table_m, c.table_scale,
                (int)c.consistent_dE, (int)c.sorted, (int)c.clf_int16, (int)c.x_exact);
    return c;
}
void fx(const char *name, const FxVerdict &v) { std::printf("%s: bits=%d k=%d why=%s\n", name, v.bits, v.k, v.why ? v.why : "-"); }

int bits_of(float v) {
    int b;
    std::memcpy(&b, &v, sizeof(b));
    return b;
}
struct Dense {
    int h[8] = {1, 1, 0, 0, 0, 1024, 1024, 0};  // not int8, not ternary, symmetric, J = +-1
    Dense(float m, int nonint, float jm = 1.0f) { h[2] = bits_of(m), h[3] = nonint, h[7] = bits_of(jm); }
    Dense &span(int hi, int lo) { return h[5] = 1024 + hi, h[6] = 1024 - lo, *this; }
};
DenseClass dense(const char *name, const Dense &d, int n = 64, int n_models = 1, int storage = SGA_J_AUTO, bool force = false) {
    const DenseClass c = classify_dense(d.h, n, n_models, storage, force);
    std::printf("%s: i8=%d tern=%d t2=%d want_i8=%d acc64=%d canon=%d table_m=%d scale=%d bits=%d clf=%d dE=%d jmax=%d\n", name,
                (int)c.fits_i8, (int)c.ternary, (int)c.use_t2, (int)c.want_i8, (int)c.acc64, (int)c.acc_canon, c.table_m, c.clf_scale,
                c.clf_bits, (int)c.clf_problem, (int)c.consistent_dE, c.j_abs_max);
    return c;
}
void ragged(const char *name, const std::vector<CsrClass> &models, RaggedOptions o) {
    const RaggedClass b = fold_ragged(models, o);
    std::printf("%s: acc=%d table_m=%d scale=%d sorted=%d clf=%d fx_bits=%d fx_k=%d why=%s\n", name, b.acc, b.table_m, b.table_scale,
                (int)b.sorted, (int)b.clf_problem, b.fx_bits, b.fx_k, b.clf_why.empty() ? "-" : b.clf_why.c_str());
}
void span_line(const char *name, const BitSpan &s) {
    if (s.any) std::printf("%s: hi=%d lo=%d\n", name, s.hi, s.lo);
    else std::printf("%s: none\n", name);
}
BitSpan span_of(std::initializer_list<float> vs) {
    BitSpan s;
    for (float v : vs) span_add(s, v);
    return s;
}

}  // namespace

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::printf("# float bit span\n");
    span_line("1.0", span_of({1.0f}));
    span_line("3.0", span_of({3.0f}));
    span_line("0.75", span_of({0.75f}));
    span_line("-0.75 and 1.0", span_of({-0.75f, 1.0f}));
    span_line("0 inf nan", span_of({0.0f, -0.0f, inf, -inf, nan}));
    span_line("2^-149", span_of({std::ldexp(1.0f, -149)}));
    span_line("3 x 2^-149", span_of({std::ldexp(3.0f, -149)}));
    span_line("largest float", span_of({std::numeric_limits<float>::max()}));
    span_line("words 0 0", span_of_words(0, 0));
    span_line("words 1044 1045", span_of_words(1044, 1045));
    std::printf("carry: %d %d %d %d %d %d\n", carry_bits(0), carry_bits(1), carry_bits(2), carry_bits(3), carry_bits(1024), carry_bits(1025));

    std::printf("# CSR integer edge\n");
    csr("16777215", scan(0, 16777215.0f, 100.0f, 0, 0));
    csr("16777216", scan(0, 16777216.0f, 100.0f, 0, 0));
    csr("below 1", scan(0, 0.5f, 0.0f, 0, 0));
    std::printf("# CSR half-integer h\n");
    csr("10.5", scan(2, 10.5f, 10.0f, 0, 0));
    csr("8388607.5", scan(2, 8388607.5f, 100.0f, 0, 0));
    csr("8388608", scan(2, 8388608.0f, 100.0f, 0, 0));
    csr("8388607.5, half_integer_table=0", scan(2, 8388607.5f, 100.0f, 0, 0), 8, 64, {false, 0});
    csr("h not a multiple of 1/2", scan(6, 100.25f, 100.0f, 0, 0));
    std::printf("# span rule\n");
    csr("CSR 42 + 10", scan(1, 10.0f, 10.0f, 20, -21), 1024);
    csr("CSR 42 + 11", scan(1, 10.0f, 10.0f, 20, -21), 1025);
    csr("CSR 43 + 10", scan(1, 10.0f, 10.0f, 20, -22), 1024);
    {
        CsrScan zero = scan(0, 16777216.0f, 0.0f, 0, 0);
        zero.exp_hi_word = zero.exp_lo_word = 0;
        csr("CSR all-zero J", zero, 0);
    }
    dense("dense 42 + 10", Dense(10.0f, 1).span(20, -21), 1024);
    dense("dense 42 + 11", Dense(10.0f, 1).span(20, -21), 1025);
    {
        const BitSpan s = span_of({std::ldexp(1.0f, 20), std::ldexp(1.0f, -21)});
        const struct { const char *name; BitSpan s; bool integral; double worst; int n; } cases[] = {
            {"TSP 42 + 10", s, false, 100.0, 256}, {"TSP 42 + 11", s, false, 100.0, 257}, {"TSP no span", BitSpan{}, false, 100.0, 2048},
            {"TSP integer 16777215", s, true, 16777215.0, 257}, {"TSP integer 16777216", s, true, 16777216.0, 257}};
        for (const auto &c : cases) {
            const TspClass t = classify_tsp(c.s, c.integral, c.worst, c.n);
            std::printf("%s: exact32=%d tsp_exact=%d\n", c.name, (int)t.exact32, (int)t.tsp_exact);
        }
    }
    std::printf("# forced classes\n");
    for (int f = 1; f <= 3; ++f) csr("table class forced", scan(0, 100.0f, 100.0f, 0, 0), 8, 64, {true, f});
    for (int f = 1; f <= 3; ++f) csr("f64 class forced", scan(1, 10.0f, 10.0f, 0, -4), 8, 64, {true, f});
    dense("exact acc64", Dense(10.0f, 1).span(0, -4));
    dense("exact acc64, force_dense_canonical", Dense(10.0f, 1).span(0, -4), 64, 1, SGA_J_AUTO, true);
    dense("integer, force_dense_canonical", Dense(10.0f, 0), 64, 1, SGA_J_AUTO, true);
    std::printf("# int16 eligibility\n");
    csr("sum |J| 32767", scan(0, 40000.0f, 32767.0f, 0, 0));
    csr("sum |J| 32768", scan(0, 40000.0f, 32768.0f, 0, 0));
    {
        CsrScan s = scan(0, 100.0f, 100.0f, 0, 0);
        s.unsorted = true;
        csr("unsorted", s);
        s.unsorted = false, s.asymmetric = true;
        csr("asymmetric", s);
        s.asymmetric = false, s.diagonal = true;
        csr("diagonal", s);
    }
    csr("n 2^30", scan(0, 100.0f, 100.0f, 0, 0), 8, 1 << 30);
    csr("n 2^30 + 1", scan(0, 100.0f, 100.0f, 0, 0), 8, (1 << 30) + 1);
    std::printf("# x_exact\n");
    csr("2^10 x 2^20 x 2^22", scan(1, 1048576.0f, 1048576.0f, -3, -22), 16, 1024);
    csr("2^10 x 2^20 x 2^23", scan(1, 1048576.0f, 1048576.0f, -3, -23), 16, 1024);
    std::printf("# fixed point, CSR\n");
    fx("2047 k 20", csr_fixed_point(classify_csr(scan(1, 2047.0f, 2047.0f, -10, -20), 16, 64, {true, 0}), 64));
    fx("2048 k 20", csr_fixed_point(classify_csr(scan(1, 2048.0f, 2048.0f, -10, -20), 16, 64, {true, 0}), 64));
    fx("2^20 k 41", csr_fixed_point(classify_csr(scan(1, 1048576.0f, 1048576.0f, -40, -41), 16, 64, {true, 0}), 64));
    fx("2^20 k 42", csr_fixed_point(classify_csr(scan(1, 1048576.0f, 1048576.0f, -40, -42), 16, 64, {true, 0}), 64));
    fx("k -2", csr_fixed_point(classify_csr(scan(0, 33554432.0f, 33554432.0f, 20, 2), 16, 64, {true, 0}), 64));
    fx("n 2^30", csr_fixed_point(classify_csr(scan(1, 10.0f, 10.0f, 0, -4), 16, 1 << 30, {true, 0}), 1 << 30));
    fx("n 2^30 + 1", csr_fixed_point(classify_csr(scan(1, 10.0f, 10.0f, 0, -4), 16, (1 << 30) + 1, {true, 0}), (1 << 30) + 1));
    {
        // reason order: canonical, unsorted, diagonal, asymmetric, width -- each case drops the reason the one before reported
        CsrScan s = scan(1, 1048576.0f, 1048576.0f, -40, -42);
        s.unsorted = s.diagonal = s.asymmetric = true;
        fx("all", csr_fixed_point(classify_csr(s, 16, 64, {true, 3}), 64));
        fx("from unsorted", csr_fixed_point(classify_csr(s, 16, 64, {true, 0}), 64));
        s.unsorted = false;
        fx("from diagonal", csr_fixed_point(classify_csr(s, 16, 64, {true, 0}), 64));
        s.diagonal = false;
        fx("from asymmetric", csr_fixed_point(classify_csr(s, 16, 64, {true, 0}), 64));
        s.asymmetric = false;
        fx("width", csr_fixed_point(classify_csr(s, 16, 64, {true, 0}), 64));
    }
    std::printf("# dense\n");
    {
        Dense i8(16777216.0f, 0);
        dense("sums 2^24, not int8", i8);
        i8.h[0] = 0;
        dense("sums 2^24, int8", i8);
        dense("sums 2^24, int8, fp32 storage", i8, 64, 1, SGA_J_F32);
        Dense t(100.0f, 0);
        t.h[0] = t.h[1] = 0;
        dense("ternary 4095", t, 4095);
        dense("ternary 4096", t, 4096);
        dense("ternary 4096, two models", t, 4096, 2);
        dense("ternary 64, bit planes asked for", t, 64, 1, SGA_J_T2);
    }
    dense("32767", Dense(32767.0f, 0));
    dense("32768", Dense(32768.0f, 0));
    dense("16383.5", Dense(16383.5f, 2));
    dense("16384", Dense(16384.0f, 2));
    dense("16777215", Dense(16777215.0f, 0));
    dense("8388607.5", Dense(8388607.5f, 2));
    dense("8388608", Dense(8388608.0f, 2));
    dense("below 1, max |J| 2.5", Dense(0.5f, 0, 2.5f));
    {
        int asked = 0;
        const auto yes = [&] { return ++asked, true; };
        const auto no = [&] { return ++asked, false; };
        Dense d(33554432.0f, 5);
        d.h[4] = 1;
        const auto why = [&](const char *name, const DenseClass &c, const std::function<bool()> &diagonal) {
            const char *text = dense_clf_why(c, diagonal);
            std::printf("clf_why %s asked=%d: %s\n", name, asked, text);
        };
        why("all", dense("not integer, h off the grid, asymmetric", d), yes);
        d.h[3] = 4;
        why("from h", classify_dense(d.h, 64, 1, SGA_J_AUTO, false), yes);
        d.h[3] = 0;
        why("diagonal", classify_dense(d.h, 64, 1, SGA_J_AUTO, false), yes);
        why("asymmetric", classify_dense(d.h, 64, 1, SGA_J_AUTO, false), no);
        d.h[4] = 0;
        why("width", classify_dense(d.h, 64, 1, SGA_J_AUTO, false), yes);
        std::printf("# fixed point, dense\n");
        asked = 0;
        Dense w(1048576.0f, 1);  // 2^20 2^42: wider than int64; span 3 + 6 carries
        w.span(-40, -42).h[4] = 1;
        fx("all", dense_fixed_point(classify_dense(w.h, 64, 2, SGA_J_AUTO, true), 2, yes));
        fx("from canonical", dense_fixed_point(classify_dense(w.h, 64, 1, SGA_J_AUTO, true), 1, yes));
        std::printf("asked=%d\n", asked);
        fx("diagonal", dense_fixed_point(classify_dense(w.h, 64, 1, SGA_J_AUTO, false), 1, yes));
        fx("asymmetric", dense_fixed_point(classify_dense(w.h, 64, 1, SGA_J_AUTO, false), 1, no));
        w.h[4] = 0;
        fx("width", dense_fixed_point(classify_dense(w.h, 64, 1, SGA_J_AUTO, false), 1, yes));
        std::printf("asked=%d\n", asked);
        fx("2^20 k 41", dense_fixed_point(classify_dense(w.span(-40, -41).h, 64, 1, SGA_J_AUTO, false), 1, yes));
        fx("2047 k 20", dense_fixed_point(classify_dense(Dense(2047.0f, 1).span(-10, -20).h, 64, 1, SGA_J_AUTO, false), 1, yes));
        fx("2048 k 20", dense_fixed_point(classify_dense(Dense(2048.0f, 1).span(-10, -20).h, 64, 1, SGA_J_AUTO, false), 1, yes));
        fx("k clamped", dense_fixed_point(classify_dense(Dense(33554432.0f, 0).span(20, 2).h, 64, 1, SGA_J_AUTO, false), 1, yes));
    }
    std::printf("# ragged fold\n");
    {
        const CsrOptions o{true, 0};
        const CsrClass t1 = classify_csr(scan(0, 10.0f, 10.0f, 0, 0), 8, 64, o), t2 = classify_csr(scan(2, 10.5f, 10.0f, 0, 0), 8, 64, o);
        const CsrClass f32 = classify_csr(scan(0, 0.5f, 0.0f, 0, 0), 8, 64, o), big = classify_csr(scan(0, 5000.0f, 5000.0f, 0, 0), 8, 64, o);
        ragged("table 1, table 2, f32", {t1, t2, f32}, {0, false, false});
        ragged("table 1, table 2", {t1, t2}, {0, false, false});
        ragged("table 2, table 1 of 5000", {t2, big}, {0, true, false});
        ragged("forced off the table", {t1, t2}, {1, true, false});
        ragged("forced off the table, fixed point", {t1, t2}, {1, true, true});
        ragged("forced canonical, fixed point", {t1, t2}, {3, true, true});
        // reason order per model: J, h, sorted, 2^15, row length, table; the first offending model wins
        CsrScan s = scan(5, 40000.0f, 32768.0f, 0, -4);
        s.unsorted = true;
        const char *names[] = {"model 1 fails all", "from h", "from sorted", "from 2^15", "from row length", "table"};
        for (int step = 0; step < 6; ++step) {
            if (step == 1) s.not_integral = 4, s.exp_lo_word = 1024;
            if (step == 2) s.not_integral = 0;
            if (step == 3) s.unsorted = false;
            if (step == 4) s.row_j_abs_max = 32767.0f;
            if (step == 5) s.not_integral = 2;  // (half-integer h, option "half_integer_table" = 0 below)
            ragged(names[step], {t1, classify_csr(s, step < 5 ? 2049 : 2048, 64, {false, 0}), classify_csr(scan(1, 10.0f, 10.0f, 0, -4), 8, 64, o)},
                   {0, true, false});
        }
        ragged("not asked", {t1, f32}, {0, false, false});
        // fixed point: canonical, sorted, row length per model; then the 2^53 bound per model at the batch-wide k
        CsrScan u = scan(1, 10.0f, 10.0f, 20, -22);
        u.unsorted = true;
        const CsrClass frac = classify_csr(scan(1, 10.0f, 10.0f, 0, -4), 8, 64, o);
        ragged("fx: model 1 canonical", {frac, classify_csr(u, 2049, 64, o), classify_csr(u, 1024, 64, o)}, {0, true, true});
        u.exp_lo_word = 1024 + 4;
        ragged("fx: model 1 unsorted, model 2 canonical", {frac, classify_csr(u, 2049, 64, o), classify_csr(scan(1, 10.0f, 10.0f, 20, -22), 1024, 64, o)}, {0, true, true});
        u.unsorted = false;
        ragged("fx: model 1 long row", {frac, classify_csr(u, 2049, 64, o)}, {0, true, true});
        ragged("fx: k 32", {classify_csr(scan(1, 1.0f, 1.0f, -30, -32), 8, 64, o), classify_csr(scan(1, 1048576.0f, 1048576.0f, 0, -5), 8, 64, o)}, {0, true, true});
        ragged("fx: k 33", {classify_csr(scan(1, 1.0f, 1.0f, -30, -33), 8, 64, o), classify_csr(scan(1, 1048576.0f, 1048576.0f, 0, -5), 8, 64, o)}, {0, true, true});
        ragged("fx: 2047 k 20", {frac, classify_csr(scan(1, 2047.0f, 2047.0f, -10, -20), 8, 64, o)}, {0, true, true});
        ragged("fx: 2048 k 20", {frac, classify_csr(scan(1, 2048.0f, 2048.0f, -10, -20), 8, 64, o)}, {0, true, true});
    }
    std::printf("# groups\n");
    {
        BitSpan g;
        groups_span_add(g, 0.5f, 3);
        groups_span_add(g, -0.375f, 2);
        groups_span_add(g, std::ldexp(1.0f, -10), 1);  // one member: no coupling
        groups_span_add(g, std::ldexp(1.0f, -12), 0);
        groups_span_add(g, 0.0f, 5);
        const struct { const char *name; BitSpan s; int word; double worst; } cases[] = {
            {"0.5 and 0.375, 2097151.875", g, 0, 2097151.875}, {"0.5 and 0.375, 2097152", g, 0, 2097152.0},
            {"remainder on 2^-5", g, 1024 + 5, 1.0}, {"remainder on 2^-1", g, 1024 + 1, 1.0}, {"nothing", BitSpan{}, 0, 16777215.0},
            {"nothing, 2^24", BitSpan{}, 0, 16777216.0}, {"2^-126", span_of({std::ldexp(1.0f, -126)}), 0, std::ldexp(1.0, -126)},
            {"2^-127", span_of({std::ldexp(1.0f, -127)}), 0, std::ldexp(1.0, -127)}};
        for (const auto &c : cases) {
            const GroupsClass r = classify_groups(c.s, c.word, c.worst);
            std::printf("%s: k=%d exact=%d\n", c.name, r.k, (int)r.exact);
        }
    }
    return 0;
}
