// window_state.cpp -- the three resets of the window forms' state (csrc/sga_windows.h, WindowState): every member is
// filled with a value that is not its default, every buffer with a distinct non-null sentinel (no device memory: the
// release function only records what it is handed), then one reset runs and the program prints which members are back
// at their defaults and which buffers were released, in the struct's order.  tests/test_window_forms_host.py holds the
// print against the lifetimes the struct declares.
#include <cstdio>
#include <string>
#include <vector>

#include "sga_windows.h"

using sga_windows::WindowState;

namespace {

std::vector<void *> g_released;
void record(void *p) { g_released.push_back(p); }

template <typename T>
T *sentinel(int i) {
    return reinterpret_cast<T *>((size_t)0x1000 * (size_t)(i + 1));
}

WindowState filled() {
    WindowState w;
    w.seq_w = 512;
    w.suspend = true;
    w.grid_planes = 3;
    w.grid_k = 2;
    w.jp = sentinel<unsigned long long>(0);
    w.jabs = sentinel<int>(1);
    w.ones = true;
    w.tiles_refused = true;
    w.seq_j8 = sentinel<int8_t>(2);
    w.seq_j8_refused = true;
    w.tuned_w = 256;
    w.tuned_rule = SGA_RULE_GLAUBER;
    w.seq_base = sentinel<int>(3);
    w.seq_base_w = 1024;
    w.rs.cnt = sentinel<int>(4);
    w.rs.off = sentinel<int>(5);
    w.rs.tot = sentinel<int>(6);
    w.rs.ent = sentinel<int>(7);
    w.rs.base = sentinel<int>(8);
    w.rs.bits = sentinel<uint32_t>(9);
    w.rs.jp = w.jp;
    w.rs.jabs = w.jabs;
    w.rs.W = 512;
    w.rs.log_w = 9;
    w.rs.nw32 = 32;
    w.rs.planes = 3;
    w.rs.log_rg = 5;
    w.rs.n_groups = 2;
    w.rs_R = 64;
    w.rs_n = 1000;
    w.rs_grid = 3;
    return w;
}

void report(const char *name, void (WindowState::*reset)(WindowState::Release)) {
    const WindowState before = filled(), fresh;
    WindowState w = filled();
    g_released.clear();
    (w.*reset)(record);
    std::string out = std::string(name) + " reset:";
    // a member is "reset" when it left its filled value for its default, and every member either did that or kept its value
    bool ok = true;
#define MEMBER(m)                                        \
    if (w.m == fresh.m) out += " " #m;                   \
    else if (!(w.m == before.m)) ok = false;
    MEMBER(seq_w) MEMBER(suspend) MEMBER(grid_planes) MEMBER(grid_k) MEMBER(jp) MEMBER(jabs) MEMBER(ones) MEMBER(tiles_refused)
    MEMBER(seq_j8) MEMBER(seq_j8_refused) MEMBER(tuned_w) MEMBER(tuned_rule) MEMBER(seq_base) MEMBER(seq_base_w) MEMBER(rs.cnt)
    MEMBER(rs.off) MEMBER(rs.tot) MEMBER(rs.ent) MEMBER(rs.base) MEMBER(rs.bits) MEMBER(rs.jp) MEMBER(rs.jabs) MEMBER(rs.W)
    MEMBER(rs.log_w) MEMBER(rs.nw32) MEMBER(rs.planes) MEMBER(rs.log_rg) MEMBER(rs.n_groups) MEMBER(rs_R) MEMBER(rs_n) MEMBER(rs_grid)
#undef MEMBER
    out += " | released:";
    const struct {
        const char *name;
        const void *p;
    } buffers[] = {{"rs.cnt", before.rs.cnt}, {"rs.off", before.rs.off}, {"rs.tot", before.rs.tot}, {"rs.ent", before.rs.ent},
                   {"rs.base", before.rs.base}, {"rs.bits", before.rs.bits}, {"seq_base", before.seq_base}, {"jp", before.jp},
                   {"jabs", before.jabs}, {"seq_j8", before.seq_j8}};
    for (void *p : g_released) {  // in the order of the calls; a pointer handed over twice shows twice
        const char *n = "?";
        for (const auto &b : buffers)
            if (b.p == p) n = b.name;
        out += std::string(" ") + n;
    }
    std::printf("%s%s\n", out.c_str(), ok ? "" : " (a member holds neither its value nor its default)");
}

}  // namespace

int main() {
    report("next_plan", &WindowState::next_plan);
    report("next_replicas", &WindowState::next_replicas);
    report("next_problem", &WindowState::next_problem);
    return 0;
}
