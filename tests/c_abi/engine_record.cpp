// engine_record.cpp -- the two resets of the engine record (csrc/sga_engine_impl.h: ProblemState, ReplicaState and what
// stays in sga_engine) without a GPU.  Every member of an sga_engine is filled with a value that is not its default, every
// pointer with a distinct non-null sentinel (no device memory: the release function only records what it is handed).
// Then free_replicas(), free_problem() or both run, and the program prints, per part of the record, the members back at
// their defaults, the members that kept their filled value, the members that hold neither, and the pointers released, in
// the order of the calls.  Argument "selfcheck": one value member and one buffer are put back after the resets, so the
// report must name them.  tests/test_engine_reuse_host.py holds the print against the declarations.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "sga_engine_impl.h"

// The members the program covers, in the order of their declarations.
#define PROBLEM_MEMBERS(M)                                                                                                  \
    M(n) M(n_models) M(shared_j) M(ragged) M(n_rows) M(model_n) M(model_row0) M(d_models) M(ragged_at) M(csr) M(want_i8)    \
    M(acc64) M(acc_canon) M(use_t2) M(J_bits) M(row_nnz) M(J_packed) M(ldj) M(rowptr) M(colidx) M(rowptr64) M(rowinfo)      \
    M(slotted) M(csr_sorted) M(cvp) M(cvp_tried) M(table_scale) M(layout_entries) M(max_row_len) M(val) M(cv) M(nnz) M(h)   \
    M(diag) M(tsp) M(tsp_exact) M(nd4) M(nd4t) M(tsp_args) M(groups) M(g_gptr) M(g_members) M(g_gent) M(g_member_ptr)       \
    M(g_coeff) M(g_rptr) M(g_rent) M(g_memberships) M(g_max_size) M(g_kmax) M(g_exp) M(group_args) M(epart) M(epart_bytes)  \
    M(tune_table) M(consistent_dE) M(from_dense) M(clf_problem) M(row_abs_max) M(j_abs_max) M(clf_csr_problem)              \
    M(clf_ragged_why) M(clf_fx_bits) M(clf_fx_k) M(clf_fx_why) M(clf_why) M(row_j_abs_max) M(csr_row_abs_max) M(hq)         \
    M(clf_scale) M(clf_bits) M(ldf) M(csr_acc) M(scan_words) M(scan_per_model) M(csr_x_exact) M(ld) M(waves) M(cpw)         \
    M(waves_t2) M(cpw_t2) M(big) M(big_form) M(table_m) M(tsp_waves) M(tsp_passes) M(csr_storage_latched)
#define REPLICA_MEMBERS(M)                                                                                                  \
    M(R) M(Rg) M(spins) M(best_spins) M(energy) M(best_energy) M(rep_temp) M(n_acc) M(n_ladders) M(slot_temps)              \
    M(slot_to_rep) M(ex_attempts) M(ex_accepts) M(wolff_u) M(wolff_cursor) M(wolff_cap) M(fields) M(fields_valid) M(ybuf)   \
    M(ybuf_bytes) M(routing) M(d_rep_lists)
#define ENGINE_MEMBERS(M)                                                                                                   \
    M(opt) M(opt_stale) M(opt_stale_key) M(caller_tune_waves) M(caller_csr_ups) M(tune_waves) M(tune_spl) M(csr_storage)    \
    M(field_cache) M(rule) M(device) M(cus) M(own_stream) M(stream) M(aux_stream) M(fork_ev) M(join_ev) M(last_kernel)      \
    M(d_count) M(d_flags) M(scratch) M(point_sites) M(point_out) M(csr_energy) M(timing) M(events) M(launches) M(total_ms)  \
    M(win.seq_w) M(win.suspend) M(replica0) M(seed) M(sstride) M(attempted) M(sweeps_done) M(rounds)

namespace {

std::vector<void *> g_released;
void record(void *p) { g_released.push_back(p); }

int g_seq = 0;                                          // every filled value differs from every other
std::vector<std::pair<const void *, std::string>> g_sentinels;  // pointer -> the member it was made for

// ---- fill: a value that is not the member's default
template <typename T>
void fill(T &v, const char *name) {
    ++g_seq;
    if constexpr (std::is_same_v<T, bool>) {
        v = !v;
    } else if constexpr (std::is_arithmetic_v<T>) {
        v = (T)(v + (T)(3 + g_seq));
    } else if constexpr (std::is_same_v<T, const char *>) {
        static const char text[] = "filled";
        v = text;
    } else if constexpr (std::is_pointer_v<T>) {
        v = reinterpret_cast<T>((uintptr_t)0x1000 * (uintptr_t)g_seq);
        g_sentinels.emplace_back(v, name);
    } else if constexpr (std::is_same_v<T, std::string>) {
        v = "filled " + std::to_string(g_seq);
    } else {
        static_assert(std::is_arithmetic_v<typename T::value_type>, "a vector of numbers");
        v.assign(3, (typename T::value_type)g_seq);
    }
}
void fill(Scratch &v, const char *name) { fill(v.ptr, name), fill(v.cap, name); }
void fill(std::vector<std::pair<hipEvent_t, hipEvent_t>> &v, const char *name) {
    v.resize(1);
    fill(v[0].first, name), fill(v[0].second, name);
}
void fill(sga::TspArgs &v, const char *name) {
    fill(v.nd4, name), fill(v.nd4t, name), fill(v.n_cities, name), fill(v.npad, name), fill(v.div_magic, name);
    fill(v.row_bytes, name), fill(v.a2, name), fill(v.b2, name), fill(v.f64, name);
}
void fill(sga::GroupArgs &v, const char *name) {
    fill(v.gptr, name), fill(v.gent, name), fill(v.member_ptr, name), fill(v.members, name), fill(v.n_groups, name);
    fill(v.wide, name), fill(v.rest.rptr, name), fill(v.rest.rent, name), fill(v.rest.nnz, name), fill(v.rest.max_row, name);
}
void fill(sga_route::ReplicaRouting &v, const char *name) {
    fill(v.route, name), fill(v.n_cached, name), fill(v.wide, name), fill(v.hot, name), fill(v.dirty, name);
    fill(v.unavailable, name), fill(v.mark_acc, name), fill(v.mark_attempted, name), fill(v.interval, name);
}
template <typename T, size_t N>
void fill(T (&v)[N], const char *name) {
    for (T &x : v) fill(x, name);
}

// ---- same: member-wise equality
template <typename T>
bool same(const T &a, const T &b) {
    return a == b;
}
bool same(const Scratch &a, const Scratch &b) { return a.ptr == b.ptr && a.cap == b.cap; }
bool same(const sga::TspArgs &a, const sga::TspArgs &b) {
    return a.nd4 == b.nd4 && a.nd4t == b.nd4t && a.n_cities == b.n_cities && a.npad == b.npad && a.div_magic == b.div_magic &&
           a.row_bytes == b.row_bytes && a.a2 == b.a2 && a.b2 == b.b2 && a.f64 == b.f64;
}
bool same(const sga::GroupArgs &a, const sga::GroupArgs &b) {
    return a.gptr == b.gptr && a.gent == b.gent && a.member_ptr == b.member_ptr && a.members == b.members &&
           a.n_groups == b.n_groups && a.wide == b.wide && a.rest.rptr == b.rest.rptr && a.rest.rent == b.rest.rent &&
           a.rest.nnz == b.rest.nnz && a.rest.max_row == b.rest.max_row;
}
bool same(const sga_route::ReplicaRouting &a, const sga_route::ReplicaRouting &b) {
    return a.route == b.route && a.n_cached == b.n_cached && a.wide == b.wide && a.hot == b.hot && a.dirty == b.dirty &&
           a.unavailable == b.unavailable && a.mark_acc == b.mark_acc && a.mark_attempted == b.mark_attempted &&
           a.interval == b.interval;
}
template <typename T, size_t N>
bool same(const T (&a)[N], const T (&b)[N]) {
    for (size_t i = 0; i < N; ++i)
        if (!same(a[i], b[i])) return false;
    return true;
}

void print(const std::string &key, const std::string &names) { std::printf("%s:%s\n", key.c_str(), names.c_str()); }

// One scenario: which resets run over a filled engine, and what the record looks like afterwards.
void report(const char *name, const sga_engine &fresh, const sga_engine &before, bool replicas, bool problem, bool selfcheck) {
    sga_engine e = before;
    g_released.clear();
    if (replicas) e.free_replicas(record);
    if (problem) e.free_problem(record);
    if (selfcheck) {
        e.table_scale = before.table_scale;
        e.g_rent = before.g_rent;
    }
    std::string reset, kept, neither;
#define MEMBER(m)                                        \
    if (same(e.m, fresh.m)) reset += " " #m;             \
    else if (same(e.m, before.m)) kept += " " #m;        \
    else neither += " " #m;
#define PART(part, LIST)                                 \
    reset = kept = neither = "";                         \
    LIST(MEMBER)                                         \
    print(std::string(name) + "." part ".reset", reset); \
    print(std::string(name) + "." part ".kept", kept);   \
    print(std::string(name) + "." part ".neither", neither);
    PART("problem", PROBLEM_MEMBERS)
    PART("replica", REPLICA_MEMBERS)
    PART("engine", ENGINE_MEMBERS)
#undef PART
#undef MEMBER
    std::string released;
    for (void *p : g_released) {  // in the order of the calls; a pointer handed over twice shows twice
        std::string n = "?";
        for (const auto &s : g_sentinels)
            if (s.first == p) n = s.second;
        released += " " + n;
    }
    print(std::string(name) + ".released", released);
    // the autotuner's pick against the caller's own values, and every other option
    bool others = true;
    for (int i = 0; i < OPT_COUNT; ++i)
        if (i != OPT_CSR_UPDATES_PER_STEP && e.opt[i] != before.opt[i]) others = false;
    std::printf("%s.caller: tune_waves=%s csr_updates_per_step=%s other_options=%s\n", name,
                e.tune_waves == before.caller_tune_waves ? "caller's" : e.tune_waves == before.tune_waves ? "kept" : "?",
                e.opt[OPT_CSR_UPDATES_PER_STEP] == before.caller_csr_ups                  ? "caller's"
                : e.opt[OPT_CSR_UPDATES_PER_STEP] == before.opt[OPT_CSR_UPDATES_PER_STEP] ? "kept"
                                                                                          : "?",
                others ? "kept" : "?");
}

}  // namespace

int main(int argc, char **argv) {
    const bool selfcheck = argc > 1 && !std::strcmp(argv[1], "selfcheck");
    const sga_engine fresh{};
    sga_engine before{};
    std::string unfilled;
#define FILL(m)             \
    fill(before.m, #m);     \
    if (same(before.m, fresh.m)) unfilled += " " #m;
#define NAME(m) names += " " #m;
    PROBLEM_MEMBERS(FILL) REPLICA_MEMBERS(FILL) ENGINE_MEMBERS(FILL)
    std::string names;
    PROBLEM_MEMBERS(NAME) print("members.problem", names), names = "";
    REPLICA_MEMBERS(NAME) print("members.replica", names), names = "";
    ENGINE_MEMBERS(NAME) print("members.engine", names);
#undef NAME
#undef FILL
    print("members.unfilled", unfilled);  // (a member whose filled value is its default would prove nothing)
    report("free_replicas", fresh, before, true, false, selfcheck);
    report("free_problem", fresh, before, false, true, selfcheck);
    report("both", fresh, before, true, true, selfcheck);  // as every setter and sga_destroy call them
    return 0;
}
