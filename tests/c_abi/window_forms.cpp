// window_forms.cpp -- the window forms' admission rules (csrc/sga_windows.h, the pure half) over trait tuples read from
// standard input; tests/test_window_forms_host.py compares the print with tests/golden/window_forms.json (the parent
// commit's answers) and with values written from the documented rules.  No device call: libsga.so is only linked for
// sga_windows.cpp and sga_route.cpp -- or sga_windows.cpp is compiled in with SGA_WINDOWS_PURE (the sanitizer build).
// One case per line, "name=value ..." over the members of WindowTraits (and lean=0|1, default 1), the rest at
// the struct's defaults.  Printed per case:
//   form=<planes>,<grid> rs_w=<W> seq=<W>,<grid>,<mode> tiles=<S>,<ones>,<why> | admit=<planes>,<grid>,<jmax> or no(<why>)
// A line "query <hex bytes of a sga_route_query>" goes through sga_route's adapter instead and prints rs_w and grid.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "sga_windows.h"
#ifndef SGA_WINDOWS_PURE
#include "sga_route.h"
#endif

using namespace sga_windows;

namespace {

bool set_trait(WindowTraits &t, const std::string &key, long long v) {
#define TRAIT(name)                      \
    if (key == #name) {                  \
        t.name = (decltype(t.name))v;    \
        return true;                     \
    }
    TRAIT(dense) TRAIT(implicit) TRAIT(ragged) TRAIT(n_models) TRAIT(shared_j) TRAIT(n) TRAIT(R) TRAIT(ldj) TRAIT(sstride)
    TRAIT(want_i8) TRAIT(acc64) TRAIT(table_m) TRAIT(j_abs_max) TRAIT(grid_planes) TRAIT(grid_k) TRAIT(consistent_dE)
    TRAIT(packed) TRAIT(rule) TRAIT(field_cache) TRAIT(cus) TRAIT(row_shared) TRAIT(row_shared_grid) TRAIT(row_shared_window)
    TRAIT(row_shared_fields) TRAIT(row_shared_tile_sites) TRAIT(look_ahead) TRAIT(force_general) TRAIT(tuned_w)
    TRAIT(tuned_rule) TRAIT(suspend) TRAIT(seq_w) TRAIT(planes_resident) TRAIT(ones) TRAIT(tiles_refused)
#undef TRAIT
    return false;
}

void print_forms(const WindowTraits &t, bool lean) {
    const WindowClass f = form_class(t), a = admission(t);
    const sga::SeqWindows q = sequential(t);
    const char *why = nullptr;
    const sga::RowSharedTiles s = tiles(t, &why);
    std::printf("form=%d,%d rs_w=%d seq=%d,%d,%d tiles=%d,%d,%s | admit=", f.planes, f.grid, row_shared_w(t, lean), q.W, q.grid, q.mode,
                s.S, s.ones, why ? why : "-");
    if (a.why) std::printf("no(%s)\n", a.why);
    else std::printf("%d,%d,%d\n", a.planes, a.grid, a.jmax);
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream in(line);
        std::string tok;
#ifndef SGA_WINDOWS_PURE
        if (line.compare(0, 6, "query ") == 0) {
            sga_route_query q;
            in >> tok >> tok;
            if (tok.size() != 2 * sizeof(q)) return std::fprintf(stderr, "query: %zu hex digits, not %zu\n", tok.size(), 2 * sizeof(q)), 2;
            for (size_t i = 0; i < sizeof(q); ++i)
                reinterpret_cast<unsigned char *>(&q)[i] = (unsigned char)std::stoi(tok.substr(2 * i, 2), nullptr, 16);
            const WindowTraits t = sga_route::window_traits_of_query(q);
            std::printf("rs_w=%d grid=%d\n", row_shared_w(t, true), form_class(t).grid);
            continue;
        }
#endif
        WindowTraits t{};
        bool lean = true;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) return std::fprintf(stderr, "not name=value: %s\n", tok.c_str()), 2;
            const std::string key = tok.substr(0, eq);
            const long long v = std::stoll(tok.substr(eq + 1));
            if (key == "lean") lean = v != 0;
            else if (!set_trait(t, key, v)) return std::fprintf(stderr, "no such trait: %s\n", key.c_str()), 2;
        }
        print_forms(t, lean);
    }
    return 0;
}
