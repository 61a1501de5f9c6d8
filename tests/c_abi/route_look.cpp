// route_look.cpp -- drives the cached-field modes' sweep-time policy (sga_route.h: look, clf_looks) over scripted
// acceptance counters and prints the state after every step; tests/test_host_logic.py compares the print with lines
// written from the thresholds.  No device call: libsga.so is only linked for sga_route.cpp.
// n = 100 spins and R = 4 replicas throughout.  theta = 0.125 is passed in directly: 0.8 theta = 0.1 and 1.2 theta =
// 0.15 are then the doubles that 40 / 400 and 60 / 400 round to, so "exactly at the threshold" can be written as counts
// (0.8 x 0.10 rounds above 8 / 100 in binary).
#include <cstdio>
#include <vector>

#include "sga_route.h"

using namespace sga_route;

namespace {

struct Script {
    ReplicaRouting s;
    LookInput in;
    std::vector<unsigned long long> acc;  // the device counters: they only grow
    explicit Script(const char *name) : acc(4, 0ull) {
        in.n = 100;
        in.R = 4;
        in.theta = 0.125;
        std::printf("# %s\n", name);
    }
    // the replicas accept d[] more proposals, the engine has attempted `attempted` per replica by then, a call starts
    void step(long long attempted, unsigned long long d0, unsigned long long d1, unsigned long long d2, unsigned long long d3) {
        const unsigned long long d[4] = {d0, d1, d2, d3};
        for (int r = 0; r < 4; ++r) acc[(size_t)r] += d[r];
        in.attempted = attempted;
        bool due = false;  // (the engine reads the counters back only when asked)
        const bool back = look(s, in, [&]() -> const unsigned long long * {
            due = true;
            return acc.data();
        });
        std::printf("at=%lld due=%d reseed=%d route=", attempted, (int)due, (int)back);
        for (int v : s.route) std::printf("%d", v);
        std::printf(" cached=%d hot=%d wide=%d interval=%d mark=%lld dirty=%d\n", s.n_cached, (int)s.hot, (int)s.wide, s.interval,
                    s.mark_attempted, (int)s.dirty);
    }
};

// which looks a cached-field call of a query takes: dense int8 rows of 6144, 16 replicas, AUTO unless said otherwise
void looks_of(const char *name, void (*change)(sga_route_query &)) {
    sga_route_query q;
    (void)sga_route_query_init(&q);
    q.kind = SGA_ROUTE_DENSE;
    q.field_cache = SGA_FIELD_CACHE_AUTO;
    q.storage = SGA_J_I8;
    q.n = q.ldj = 6144;
    q.R_local = 16;
    q.cus = 256;
    q.opt[sga_impl::OPT_CLF_WAVES] = 0;
    q.opt[sga_impl::OPT_CLF_TAIL_WAVES] = 1;
    q.opt[sga_impl::OPT_CLF_BATCHED] = 2;
    change(q);
    const ClfLooks l = clf_looks(q);
    std::printf("%s: auto=%d tail=%d adaptive=%d any=%d pieces=%d\n", name, (int)l.is_auto, (int)l.tail, (int)l.adaptive, (int)l.any(),
                (int)clf_looks(q, false).any());
}

}  // namespace

int main() {
    std::printf("# clf_looks\n");
    looks_of("int8 6144 x 16", [](sga_route_query &) {});
    looks_of("15 replicas", [](sga_route_query &q) { q.R_local = 15; });
    looks_of("rows of 6016", [](sga_route_query &q) { q.ldj = 6016; });                 // fewer than six chunks
    looks_of("rows of 13312", [](sga_route_query &q) { q.ldj = 13312; });               // eight waves as it is
    looks_of("fp32 rows of 1536", [](sga_route_query &q) { q.storage = SGA_J_F32, q.ldj = 1536; });
    looks_of("fp32 rows of 1408", [](sga_route_query &q) { q.storage = SGA_J_F32, q.ldj = 1408; });
    looks_of("clf_waves=4", [](sga_route_query &q) { q.opt[sga_impl::OPT_CLF_WAVES] = 4; });
    looks_of("clf_batched=1", [](sga_route_query &q) { q.opt[sga_impl::OPT_CLF_BATCHED] = 1; });
    looks_of("CSR", [](sga_route_query &q) { q.kind = SGA_ROUTE_CSR; });
    looks_of("CSR ON", [](sga_route_query &q) { q.kind = SGA_ROUTE_CSR, q.field_cache = SGA_FIELD_CACHE_ON; });
    looks_of("ON, no look enabled", [](sga_route_query &q) {
        q.field_cache = SGA_FIELD_CACHE_ON, q.opt[sga_impl::OPT_CLF_TAIL_WAVES] = 0, q.opt[sga_impl::OPT_CLF_BATCHED] = 0;
    });
    // (the tail look armed on a launch too small for it: no look is taken, the call is still cut into pieces)
    looks_of("ON, 15 replicas, clf_batched=0", [](sga_route_query &q) {
        q.field_cache = SGA_FIELD_CACHE_ON, q.R_local = 15, q.opt[sga_impl::OPT_CLF_BATCHED] = 0;
    });
    {
        Script t("per-replica AUTO");
        t.in.looks.is_auto = true;
        t.step(400, 60, 61, 61, 50);     // r0 at exactly 1.2 theta stays, r1 and r2 above it leave, r3 between stays
        t.step(1200, 96, 80, 96, 0);     // r1 at exactly 0.8 theta stays on the rows, r2 between stays, r0 between stays
        t.step(2800, 0, 159, 160, 0);    // r1 below 0.8 theta returns: reseed
    }
    {
        Script t("whole-launch AUTO");
        t.in.looks.is_auto = true;
        t.in.per_replica = false;
        t.in.start_cached = false;
        t.step(400, 40, 10, 0, 0);       // hottest at exactly 0.8 theta: stays on the rows
        t.step(1200, 79, 0, 0, 79);      // below: every replica cached, reseed
        t.step(2800, 10, 239, 0, 0);     // between: stays
        t.step(4400, 0, 0, 240, 0);      // hottest reaches 1.2 theta: every replica back on the rows
    }
    {
        Script t("whole-launch AUTO, ragged shares 1.0 0.5 1.0 0.5");
        const int spins[4] = {100, 50, 100, 50};
        t.in.looks.is_auto = true;
        t.in.per_replica = false;
        t.in.start_cached = false;
        t.in.spins = spins;
        t.step(400, 0, 20, 0, 0);        // r1 made half the attempts: 20 counts as 40 / 400 = 0.8 theta, stays on the rows
        t.step(1200, 79, 0, 0, 39);      // 79 / 800 and 2 x 39 / 800 are below it: cached
    }
    {
        Script t("adaptive hot / cold (ON)");
        t.in.looks.adaptive = true;
        t.step(10000, 101, 0, 3, 0);     // 0.0101: stays hot
        t.step(20000, 5, 100, 0, 0);     // 0.0100: cold
        t.step(30000, 0, 0, 150, 0);     // 0.0150: stays cold
        t.step(40000, 0, 0, 0, 151);     // above: hot
    }
    {
        Script t("adaptive, a replica on the rows is not counted (AUTO)");
        t.in.looks.is_auto = true;
        t.in.looks.adaptive = true;
        t.step(10000, 100, 5000, 0, 0);  // r1 leaves; the hottest CACHED replica is at 0.0100: cold
        t.step(20000, 150, 9000, 0, 0);  // r1 stays on the rows and is not looked at: 0.0150 stays cold
    }
    {
        Script t("tail (ON)");
        t.in.looks.tail = true;
        t.step(400, 96, 12, 12, 12);     // 24 accepts per sweep, mean / hottest 0.34: not entered
        t.step(1200, 192, 8, 8, 6);      // 24 per sweep, 0.2786: entered
        t.step(2800, 384, 56, 56, 54);   // 0.3581: kept
        t.step(4400, 400, 64, 64, 48);   // 25 per sweep, 9 / 25 = 0.36: dropped
    }
    {
        Script t("tail, 23 accepts per sweep (ON)");
        t.in.looks.tail = true;
        t.step(400, 92, 0, 0, 0);
    }
    {
        Script t("tail while adaptive and hot (ON)");
        t.in.looks.tail = true;
        t.in.looks.adaptive = true;
        t.step(400, 96, 4, 4, 3);
    }
    {
        Script t("cadence");
        t.in.looks.is_auto = true;
        t.step(0, 0, 0, 0, 0);           // the first call: initial routes, no look
        t.s.dirty = false;               // (the engine has uploaded the replica lists)
        t.step(399, 1, 1, 1, 1);         // one attempt short of 4 sweeps
        t.step(400, 0, 0, 0, 0);
        t.step(1199, 0, 0, 0, 0);        // ... of 8
        t.step(1200, 0, 0, 0, 0);
        t.step(2799, 0, 0, 0, 0);        // ... of 16
        t.step(2800, 0, 0, 0, 0);
        t.step(4399, 0, 0, 0, 0);        // ... of 16 again
        t.step(4400, 0, 0, 0, 0);
        t.s.dirty = false;
        t.step(100, 0, 99, 0, 0);        // the attempts counter went backwards: only the marks move
        t.in.R = 3;                      // another replica count: from the initial routes
        t.in.start_cached = false;
        t.step(200, 0, 0, 0, 0);
    }
    return 0;
}
