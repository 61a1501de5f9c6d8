"""Every exact-integer sweep form at the limit of its number range (tests/range_edges.py): the instance whose extreme
field is the LAST value the form's set-time condition admits must run the form, its twin one unit beyond must not, and
both must walk the oracle's chain bit for bit from explicit spins (xi, -xi, xi with site 0 flipped, random) at
T = 0, L/8, L/2, 2L and inf.  tests/test_range_edges_host.py shows from the reference alone that the runs contain
the moves at the limit."""
import numpy as np
import pytest

import oracle
import range_edges as re_

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def compare(e, out, ref, trace=False):
    """Spins, tracked energies, energy trace, accept counters, per-replica bests -- then from-scratch energies."""
    R = ref["spins"].shape[0]
    assert np.array_equal(out["energy_trace"], ref["energy_trace"]), e.describe()
    assert np.array_equal(e.spins(), ref["spins"])
    assert np.array_equal(e.energies(), ref["energy"])
    assert np.array_equal(e.stats()[0], ref["n_accepted"])
    for r in range(R):
        be, bs, _ = e.best(r)
        assert be == ref["best_energy"][r] and np.array_equal(bs, ref["best_spins"][r]), r
    if trace:
        assert np.array_equal(out["accept_trace"], ref["accept_trace"])
        assert np.array_equal(out["dE_trace"], ref["dE_trace"])
    e.recompute_energies()
    assert np.array_equal(e.energies(), ref["scratch"])


def start(e, c):
    e.init_replicas(c["s0"].shape[0], seed=c["seed"], s0=c["s0"])
    e.set_temperatures(c["temps"])


def traits_match(e, want):
    q = e.route_query()
    for k, v in want.items():
        assert getattr(q, k) == v, (k, getattr(q, k), v)


# ----------------------------------------------------------------------------- 1. dense fields int16 <-> int32 at 2^15
@pytest.mark.parametrize("storage", ["f32", "i8"])
@pytest.mark.parametrize("name,bits", [("i16_in", 16), ("i16_out", 32), ("i16h_in", 16), ("i16h_out", 32)])
def test_dense_cached_fields_at_the_int16_limit(sg, name, bits, storage):
    from spin_glass_anneal_rl_amd.engine import last_kernel
    c, ref = re_.dense_case(name), re_.reference(name)
    for batched in (0, 1):
        with sg.AnnealEngine(0) as e:
            e.set_option("clf_batched", batched)
            e.set_field_cache("on")
            e.set_dense(c["J"], c["h"], storage=storage)
            start(e, c)
            traits_match(e, re_.dense_traits(c["J"], c["h"], storage))
            assert f"sweep=cached-local-fields(int{bits} in LDS" in e.describe(), e.describe()
            assert f"cached-local-fields(int{48 - bits} " not in e.describe()
            out = e.sweep(c["sweeps"], energy_trace=True)
            assert last_kernel().startswith("sweep_clfb_kernel" if batched else "sweep_clf_kernel"), last_kernel()
            compare(e, out, ref)


def test_one_accept_moves_a_field_across_the_int16_range(sg):
    c, ref = re_.dense_case("single"), re_.reference("single")
    acc = ref["accept_trace"].astype(bool)
    assert acc.any()
    for batched in (0, 1):
        with sg.AnnealEngine(0) as e:
            e.set_option("clf_batched", batched)
            e.set_field_cache("on")
            e.set_dense(c["J"], c["h"], storage="f32")
            start(e, c)
            assert "sweep=cached-local-fields(int16 in LDS" in e.describe(), e.describe()
            compare(e, e.sweep(c["sweeps"], energy_trace=True), ref)
    with sg.AnnealEngine(0) as e:  # the general build: per-update records
        e.set_field_cache("on")
        e.set_dense(c["J"], c["h"], storage="f32")
        start(e, c)
        compare(e, e.sweep(c["sweeps"], energy_trace=True, trace=True), ref, trace=True)


# ----------------------------------------------------------------------------- 2. dense fields int32 <-> refused at 2^24
@pytest.mark.parametrize("name,served", [("i24_in", True), ("i24_out", False), ("i24h_in", True), ("i24h_out", False)])
def test_dense_cached_fields_at_the_int32_limit(sg, name, served):
    from spin_glass_anneal_rl_amd.engine import last_kernel
    c, ref = re_.dense_case(name), re_.reference(name)
    want = re_.dense_traits(c["J"], c["h"], "f32")
    assert want["clf_ok"] == int(served)
    for batched in (0, 1):
        with sg.AnnealEngine(0) as e:
            e.set_option("clf_batched", batched)
            e.set_field_cache("on")
            e.set_dense(c["J"], c["h"], storage="f32")
            start(e, c)
            traits_match(e, want)
            if served:
                assert "sweep=cached-local-fields(int32 in LDS" in e.describe(), e.describe()
                out = e.sweep(c["sweeps"], energy_trace=True)
                assert last_kernel().startswith("sweep_clfb_kernel" if batched else "sweep_clf_kernel"), last_kernel()
                compare(e, out, ref)
            else:
                with pytest.raises(sg.AnnealingError, match="cached local fields") as err:
                    e.sweep(1)
                assert err.value.details["code"] == sg._native.ERR_UNSUPPORTED
                e.set_field_cache("auto")  # the streaming kernels, the oracle's chain
                assert "cached-local-fields" not in e.describe()
                out = e.sweep(c["sweeps"], energy_trace=True)
                assert last_kernel().startswith("sweep_dense_kernel"), last_kernel()
                compare(e, out, ref)


@pytest.mark.parametrize("look_ahead", [1, 0])
@pytest.mark.parametrize("name,acc", [("i24_in", "f32"), ("i24_out", "f64-exact"), ("i24h_in", "f32"), ("i24h_out", "f32")])
def test_streaming_accumulation_class_at_the_fp32_limit(sg, name, acc, look_ahead):
    """Cache off: fp32 row sums while max_i (sum_j |J_ij| + |h_i|) < 2^24, fp64 from 2^24 on (half-integer h: the bound
    is 2^23 on either side of that twin, fp32 both)."""
    from spin_glass_anneal_rl_amd.engine import last_kernel
    c, ref = re_.dense_case(name), re_.reference(name)
    with sg.AnnealEngine(0) as e:
        e.set_option("look_ahead", look_ahead)
        e.set_field_cache("off")
        e.set_dense(c["J"], c["h"], storage="f32")
        start(e, c)
        assert f" acc={acc} " in e.describe(), e.describe()
        out = e.sweep(c["sweeps"], energy_trace=True)
        assert last_kernel().startswith("sweep_dense_kernel"), last_kernel()
        compare(e, out, ref)


# ----------------------------------------------------------------------------- 3. several accepts per round, max |J| = 2^18
@pytest.mark.parametrize("jmax", [(1 << 18) - 1, 1 << 18])
def test_several_accepts_per_round_at_the_filter_limit(sg, jmax):
    """The round filter of sweep_clfb_kernel is on below max |J| = 2^18 and switches itself off from there (not visible from
    outside: the form runs on both sides, int32 fields); the hot replicas commit several accepts per round."""
    from spin_glass_anneal_rl_amd.engine import last_kernel
    J, h, xi = re_.saturating_dense(4000000, 1, None, 67)
    J[0, 1] = J[1, 0] = float(jmax) * xi[0] * xi[1]
    s0 = re_.start_spins(xi, 5, 9)
    temps = re_.temperatures(5, 4000000.0)
    ref = re_.flat_reference(J, h, s0, temps, 4, 9)
    assert ref["n_accepted"][4] == 4 * 67 and ref["n_accepted"][3] > 67
    with sg.AnnealEngine(0) as e:
        e.set_option("clf_batched", 1)
        e.set_field_cache("on")
        e.set_dense(J, h, storage="f32")
        e.init_replicas(5, seed=9, s0=s0)
        e.set_temperatures(temps)
        assert "sweep=cached-local-fields(int32 in LDS" in e.describe(), e.describe()
        out = e.sweep(4, energy_trace=True)
        assert last_kernel().startswith("sweep_clfb_kernel"), last_kernel()
        compare(e, out, ref)


# ----------------------------------------------------------------------------- 4. CSR dynamic fields at 2^15
def test_csr_cached_fields_at_the_int16_limit(sg):
    from spin_glass_anneal_rl_amd.engine import last_kernel
    for name, served in (("c16_in", True), ("c16_out", False)):
        c, ref = re_.csr_case(name), re_.reference(name)
        with sg.AnnealEngine(0) as e:
            e.set_field_cache("on")
            e.set_csr(*c["csr"], c["h"])
            start(e, c)
            traits_match(e, {k: v for k, v in re_.csr_traits(c["csr"], c["h"]).items() if k in ("clf_ok", "table_m", "acc")})
            if served:
                assert "sweep=cached-local-fields(int16 dynamic fields" in e.describe(), e.describe()
                out = e.sweep(c["sweeps"], energy_trace=True)
                assert last_kernel().startswith("sweep_clf_csr_kernel"), last_kernel()
                compare(e, out, ref)
            else:
                with pytest.raises(sg.AnnealingError, match=r"max_i sum_j \|J_ij\| < 2\^15"):
                    e.sweep(1)
                e.set_field_cache("auto")
                out = e.sweep(c["sweeps"], energy_trace=True)
                assert not last_kernel().startswith("sweep_clf_csr_kernel"), last_kernel()
                assert "cached-local-fields" not in e.describe()
                compare(e, out, ref)
        with sg.AnnealEngine(0) as e:  # traced: the general build on the row-per-proposal kernels
            e.set_csr(*c["csr"], c["h"])
            start(e, c)
            compare(e, e.sweep(c["sweeps"], energy_trace=True, trace=True), ref, trace=True)


@pytest.mark.parametrize("name", ["t2048", "t2049"])
def test_accept_table_edge_of_the_csr_rows_form(sg, name):
    """table_scale * csr_row_abs_max = 2048: the table covers every move and the several-updates-per-step form runs
    without its beyond-the-table path; 2049: one move (k = 2049, site 0 at xi) lies beyond table_m = 2048 and k = 2048 is
    the table's last entry.  Which of the two builds ran is not named by last_kernel(); the host file pins the condition
    on the instances, this test the chain on both sides, on every CSR form of these rows."""
    from spin_glass_anneal_rl_amd.engine import last_kernel
    c, ref = re_.csr_case(name), re_.reference(name)
    for ups, kernel in ((-1, "sweep_csr_rows_kernel"), (0, "sweep_csr_kernel")):
        with sg.AnnealEngine(0) as e:
            if ups >= 0:
                e.set_option("csr_updates_per_step", ups)
            e.set_csr(*c["csr"], c["h"])
            start(e, c)
            traits_match(e, {k: v for k, v in re_.csr_traits(c["csr"], c["h"]).items() if k in ("clf_ok", "table_m", "acc")})
            assert "path=integer-fast table_m=2048" in e.describe(), e.describe()
            out = e.sweep(c["sweeps"], energy_trace=True)
            assert last_kernel().startswith(kernel), last_kernel()
            compare(e, out, ref)
    with sg.AnnealEngine(0) as e:  # the cached-field form reads the same table
        e.set_field_cache("on")
        e.set_csr(*c["csr"], c["h"])
        start(e, c)
        out = e.sweep(c["sweeps"], energy_trace=True)
        assert last_kernel().startswith("sweep_clf_csr_kernel"), last_kernel()
        compare(e, out, ref)


# ----------------------------------------------------------------------------- 5. fixed-point fields int32 <-> int64 at 2^31
@pytest.mark.parametrize("kind", ["dense", "csr"])
@pytest.mark.parametrize("name,bits,rules", [("fx_in", 32, (0, 1)), ("fx_out", 64, (0,))])
def test_fixed_point_fields_at_the_int32_limit(sg, name, bits, rules, kind):
    """Option "clf_fixed_point", dyadic couplings in multiples of 2^-8: 2^8 max_i sum_j |J_ij| = 2^31 - 1984 is the largest
    bound the scan's condition (fp32 rounding, margin 1 + 2^-20) keeps in int32, 2^31 - 1983 the first it gives int64.
    From xi the field of site 0 is the bound itself.  Metropolis, and Glauber on the int32 side."""
    c = re_.dense_case(name)
    for rule in rules:
        ref = re_.reference(name, rule=rule, as_csr=kind == "csr")
        with sg.AnnealEngine(0) as e:
            e.set_option("clf_fixed_point", 1)
            e.set_field_cache("on")
            if kind == "csr":
                e.set_csr(*re_.csr_of(c["J"]), c["h"])
            else:
                e.set_dense(c["J"], c["h"], storage="f32")
            start(e, c)
            e.set_update_rule(rule)
            q = e.route_query()
            assert q.clf_bits == bits == re_.fixed_point_traits(c["J"], kind == "csr")["clf_bits"]
            assert f"int{bits} fixed-point" in e.describe() and f"k={re_.FX_K}," in e.describe(), e.describe()
            assert f"int{96 - bits} fixed-point" not in e.describe()
            out = e.sweep(c["sweeps"], energy_trace=True)
            k = e.last_kernel()
            assert k.startswith("sweep_clf_csr_kernel" if kind == "csr" else "sweep_clf_fx_kernel") and f"int{bits} fixed-point" in k, k
            compare(e, out, ref)


# ----------------------------------------------------------------------------- 6. group sums int16 <-> int32 at 2^15 members
@pytest.mark.parametrize("with_rest", [False, True])
@pytest.mark.parametrize("big_coeff", [False, True])
@pytest.mark.parametrize("G,sums", [(32767, "int16"), (32768, "int32")])
def test_group_sums_at_the_int16_limit(sg, G, sums, big_coeff, with_rest):
    """A group of 2^15 - 1 | 2^15 members, aligned at the start (S_g = +-|g|): production kernels at 1 and 2 waves, the
    traced general kernel and the from-scratch energy kernel, against the group-sum chain (no J is materialised).  The
    energy kernel records no name: that energy_groups_kernel<true, *> ran is shown by describe() -- its launcher picks the
    instantiation by the same flag that prints "group sums as int32" -- and by init_replicas' and recompute_energies'
    energies of |E| ~ 10^11 equal to the exact reference's."""
    prob, (n, groups, coeff, h, rest), s0, temps = re_.big_group(G, big_coeff, with_rest)
    ref = re_.big_group_reference(G, big_coeff, with_rest)
    other = "int32" if sums == "int16" else "int16"
    tail = ", stored remainder>" if with_rest else ">"
    for waves, trace in ((1, False), (2, False), (0, True)):
        with sg.AnnealEngine(0) as e:
            if waves:
                e.set_tuning(waves_per_replica=waves)
            e.set_groups(n, groups, coeff, h, rest=rest)
            e.init_replicas(re_.GROUPS_R, seed=re_.GROUPS_SEED, s0=s0)
            e.set_temperatures(temps)
            assert f"group sums as {sums} in LDS" in e.describe() and f"largest_group={G} " in e.describe(), e.describe()
            assert f"sums={sums} " in e.explain_route()
            assert np.array_equal(e.energies(), [prob.energy(s0[r]) for r in range(re_.GROUPS_R)])
            out = e.sweep(re_.GROUPS_SWEEPS, energy_trace=True, trace=trace)
            k = e.last_kernel()
            if trace:
                assert k.startswith(f"sweep_groups_general_kernel<{sums} sums{tail}"), k
            else:
                assert k.startswith(f"sweep_groups_kernel<{sums} sums{tail} x {waves} wave"), k
            assert other not in k
            compare(e, out, ref, trace=trace)


# ----------------------------------------------------------------------------- 7. row-shared windows: planes at |J| = 1 / 7 / 255
@pytest.mark.parametrize("R", [3, 130])
@pytest.mark.parametrize("amp,planes", [(1, 1), (7, 3), (8, 8), (255, 8), (256, 0)])
def test_row_shared_plane_counts_at_their_limits(sg, amp, planes, R):
    from spin_glass_anneal_rl_amd.engine import last_kernel
    n, seed, ns = 257, 3, 2
    J, h, xi = re_.flat_dense(amp, n)
    s0 = re_.start_spins(xi, R, seed)
    temps = re_.temperatures(R, float(amp * (n - 1) + 1))
    ref = re_.flat_reference(J, h, s0, temps, ns, seed)
    with sg.AnnealEngine(0) as e:
        e.set_option("row_shared", 1)
        e.set_option("row_shared_window", 256)
        e.set_dense(J, h, storage="f32")
        e.init_replicas(R, seed=seed, s0=s0)
        e.set_temperatures(temps)
        if planes:
            assert f"sweep=row-shared(W=256 planes={planes})" in e.describe(), e.describe()
        else:
            assert "row-shared" not in e.describe(), e.describe()
        out = e.sweep(ns, energy_trace=True)
        assert last_kernel().startswith("sweep_dense_rs<") == bool(planes), last_kernel()
        if planes:
            assert f"planes={planes}," in last_kernel(), last_kernel()
        compare(e, out, ref)


# ----------------------------------------------------------------------------- 8. int8 rows at |J| = 127
@pytest.mark.parametrize("look_ahead", [1, 0])
def test_int8_rows_at_their_limit(sg, look_ahead):
    from spin_glass_anneal_rl_amd.engine import last_kernel
    n, R, seed, ns = 261, 5, 4, 2
    for spike in (None, 128):
        J, h, xi = re_.flat_dense(127, n, spike)
        s0 = re_.start_spins(xi, R, seed)
        temps = re_.temperatures(R, float(127 * (n - 1) + 1))
        ref = re_.flat_reference(J, h, s0, temps, ns, seed)
        with sg.AnnealEngine(0) as e:
            e.set_option("look_ahead", look_ahead)
            if spike:
                with pytest.raises(sg.AnnealingError, match="int8 storage requested"):
                    e.set_dense(J, h, storage="i8")
            e.set_dense(J, h, storage="auto" if spike else "i8")
            e.init_replicas(R, seed=seed, s0=s0)
            e.set_temperatures(temps)
            assert (" storage=f32 " if spike else " storage=i8 ") in e.describe(), e.describe()
            out = e.sweep(ns, energy_trace=True)
            assert last_kernel().startswith("sweep_dense_kernel"), last_kernel()
            compare(e, out, ref)


def test_packed_csr_entries_at_their_limit(sg):
    """A degree-300 graph (64-entry slots, the bit-spin wide form) with every |J| = 127: packed 32-bit entries, required and
    by default.  One coupling of 128: "packed" fails at init_replicas, "auto" keeps the (column, value) entries."""
    R, seed, ns = 5, 6, 2
    for spike in (None, 128):
        csr, h, xi, J = re_.packed_csr(spike)
        s0 = re_.start_spins(xi, R, seed)
        temps = re_.temperatures(R, float(np.abs(J).sum(1).max() + 1))
        prob = oracle.Problem(csr=csr, h=h)
        s = s0.copy()
        ref = oracle.sweeps(prob, s, temps, ns, seed=seed, n_threads=5)
        ref["spins"], ref["scratch"] = s, oracle.energy(prob, s)
        assert not ref["n_accepted"][0] and np.array_equal(s[0], xi)   # T = 0 at xi: every row at 127 x 300 throughout
        for storage in ("packed", "auto"):
            with sg.AnnealEngine(0) as e:
                e.set_option("force_csr_bits", 1)
                e.set_tuning(waves_per_replica=2)
                e.set_csr_storage(storage)
                e.set_csr(*csr, h)
                if spike and storage == "packed":
                    with pytest.raises(sg.AnnealingError):
                        e.init_replicas(R, seed=seed, s0=s0)
                    continue
                e.init_replicas(R, seed=seed, s0=s0)
                e.set_temperatures(temps)
                assert ("entries=packed-32bit" in e.describe()) == (spike is None), e.describe()
                assert e.route_query().packed_ok == re_.packed_traits(csr)["packed_ok"]
                assert ("entries=packed " in e.explain_route()) == (spike is None), e.explain_route()
                out = e.sweep(ns, energy_trace=True)
                assert "one replica per workgroup, bit spins" in e.last_kernel(), e.last_kernel()
                compare(e, out, ref)
