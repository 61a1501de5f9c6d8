"""The range-edge instances of tests/range_edges.py do what they claim, shown by the reference alone; the group-sum
reference equals the oracle where both can run; and the form each side of every twin takes, by csrc/sga_route.cpp on the
traits the set-time scans would find (no device)."""
import numpy as np
import pytest

import groups_cases as gc
import oracle
import range_edges as re_

SATURATING = list(re_.DENSE) + ["single", "c16_in", "c16_out", "t2048", "t2049"]


@pytest.mark.parametrize("name", SATURATING)
def test_the_instance_sits_at_its_limit(name):
    c = re_.case(name)
    ref, dE, s = re_.proposals(c["J"], c["h"], c["s0"], c["temps"], c["sweeps"], c["seed"])
    assert np.array_equal(s, re_.reference(name)["spins"])
    # the move at the limit: site 0 in state xi.  (CSR: the limit is on the dynamic part J s alone, |h_0| rides on top.)
    top = 2.0 * (c["L"] / c["scale"] + (abs(float(c["h"][0])) if name.startswith("c16") else 0.0))
    one = 4.0 * float(np.abs(c["J"]).max())  # one flipped coupling moves a field by 2 |J|, dE by 4 |J|
    assert (dE == top).any() and (dE == -top).any(), name            # exactly at the limit, both signs
    assert ((np.abs(dE) < top) & (np.abs(dE) >= top - one)).any(), name   # within one coupling of it
    assert np.abs(dE).max() == top                                   # and nothing beyond
    acc = ref["accept_trace"].astype(bool)
    for r, T in enumerate(c["temps"]):
        if 0.0 < T < re_.INF:
            assert acc[r].any() and not acc[r].all(), (name, r)
    assert c["temps"][0] == 0.0 and not acc[0].any()                 # T = 0 at xi: the field stays at +L throughout
    assert np.array_equal(s[0], c["xi"])
    assert c["temps"][4] == re_.INF and acc[4].all()


def test_row_bounds_are_exact_and_distinct():
    for name in re_.DENSE:
        c = re_.dense_case(name)
        b = c["scale"] * (np.abs(c["J"]).astype(np.float64).sum(1) + np.abs(c["h"]))
        assert b[0] == c["L"] and (b[1:] < c["L"]).all() and np.unique(b).size == b.size and c["J"].shape[0] % 64
        assert np.array_equal(c["J"], c["J"].T) and not np.diag(c["J"]).any()
        if re_.DENSE[name][2]:  # int8 rows: the bound is reached with the storage's largest coupling
            assert np.abs(c["J"]).max() == 127
    for name in ("c16_in", "c16_out"):
        c = re_.csr_case(name)
        mj = np.abs(c["J"]).astype(np.float64).sum(1)
        assert mj[0] == c["L"] and (mj[1:] < c["L"]).all() and np.abs(c["h"]).min() >= 3 * 32768
    J, h, xi = re_.single_coupling_dense()
    assert np.count_nonzero(J[0]) == 1 and abs(J[0, 1]) == 32766 and abs(h[0]) == 1


@pytest.mark.parametrize("name", ["scheduling_6x1x12", "big_n700"])
def test_group_sum_reference_equals_the_oracle(name):
    n, mp, mem, c, h, csr = gc.problem(name)
    temps = gc.ladder(4)
    s1 = oracle.init_spins(n, 4, gc.SEED)
    s2 = s1.copy()
    want = oracle.sweeps(oracle.Problem(h=h, csr=csr), s1, temps, 4, seed=gc.SEED, trace=True)
    P = re_.GroupProblem(n, mp, mem, c, h)
    got = P.sweeps(s2, temps, 4, gc.SEED)
    for key in ("energy", "energy_trace", "n_accepted", "best_energy", "best_spins", "accept_trace", "dE_trace"):
        assert np.array_equal(want[key], got[key]), key
    assert np.array_equal(s1, s2) and 0 < want["n_accepted"].sum() < 16 * n
    assert np.array_equal([P.energy(s2[r]) for r in range(4)], oracle.energy(oracle.Problem(h=h, csr=csr), s2))


def test_group_sum_reference_with_a_remainder_equals_the_oracle():
    import groups_rest_cases as grc
    n, mp, mem, c, rest, h, csr = grc.problem("big_n700_rest")
    temps = gc.ladder(3)
    s1 = oracle.init_spins(n, 3, gc.SEED)
    s2 = s1.copy()
    want = oracle.sweeps(oracle.Problem(h=h, csr=csr), s1, temps, 3, seed=gc.SEED, trace=True)
    got = re_.GroupProblem(n, mp, mem, c, h, rest).sweeps(s2, temps, 3, gc.SEED)
    for key in ("energy", "energy_trace", "n_accepted", "accept_trace", "dE_trace"):
        assert np.array_equal(want[key], got[key]), key
    assert np.array_equal(s1, s2)


# ----------------------------------------------------------------------------- route pins (strings: csrc/sga_route.cpp)
def explain(**fields):
    from spin_glass_anneal_rl_amd import _native as N
    return N.explain_route(N.route_query(**fields))


@pytest.mark.parametrize("twin,bits", [("i16", (16, 32)), ("i16h", (16, 32))])
def test_route_dense_field_width(twin, bits):
    for side, b in zip(("_in", "_out"), bits):
        c = re_.dense_case(twin + side)
        for storage in ("f32", "i8"):
            t = re_.dense_traits(c["J"], c["h"], storage)
            assert t["clf_ok"] == 1 and t["clf_bits"] == b and t["clf_scale"] == c["scale"]
            assert f"fields=int{b})" in explain(R_local=5, field_cache=1, **t)


@pytest.mark.parametrize("twin", ["i24", "i24h"])
def test_route_dense_served_or_refused_and_accumulation_class(twin):
    a, b = (re_.dense_case(twin + s) for s in ("_in", "_out"))
    ta, tb = re_.dense_traits(a["J"], a["h"]), re_.dense_traits(b["J"], b["h"])
    assert (ta["clf_ok"], ta["clf_bits"], tb["clf_ok"]) == (1, 32, 0)
    assert "cached=on(" in explain(R_local=5, field_cache=1, **ta) and "fields=int32)" in explain(R_local=5, field_cache=1, **ta)
    assert explain(R_local=5, field_cache=1, **tb).endswith("cached=refused")
    assert explain(R_local=5, field_cache=2, **tb).endswith("cached=unavailable")
    # the streaming kernels' accumulation: fp32 while m < 2^24 (integer J), fp64 from 2^24 on
    if twin == "i24":
        assert (ta["acc"], tb["acc"]) == (0, 1)
        assert " acc=f32 " in explain(R_local=5, **ta) and " acc=f64-exact " in explain(R_local=5, **tb)
    else:  # scale 2: m = 2^23 - 1/2 | 2^23 -- the row sums stay far below 2^24 on both sides
        assert (ta["acc"], tb["acc"]) == (0, 0)


def test_route_csr_dynamic_fields():
    a, b = re_.csr_case("c16_in"), re_.csr_case("c16_out")
    ta, tb = re_.csr_traits(a["csr"], a["h"]), re_.csr_traits(b["csr"], b["h"])
    assert (ta["clf_ok"], tb["clf_ok"]) == (1, 0) and ta["table_m"] == tb["table_m"] == 2048
    assert "cached=on(waves=" in explain(R_local=5, field_cache=1, **ta)
    assert explain(R_local=5, field_cache=1, **tb).endswith("cached=refused")
    assert explain(R_local=5, field_cache=2, **tb).endswith("cached=unavailable")


def test_route_group_sums():
    for G, sums in ((32767, "int16"), (32768, "int32")):
        prob, (n, (mp, mem), coeff, h, rest), s0, temps = re_.big_group(G, False, False)
        text = explain(kind=3, n=n, n_groups=coeff.size, group_max=int(np.diff(mp).max()), R_local=4)
        assert f"largest_group={G} sums={sums} " in text, text


def test_route_packed_entries():
    a, b = re_.packed_traits(re_.packed_csr()[0]), re_.packed_traits(re_.packed_csr(128)[0])
    assert (a["packed_ok"], b["packed_ok"]) == (1, 0) and a["max_row_len"] == 300 and a["nnz"] / a["n"] >= 192
    assert "form=wide-bits " in explain(**a) and " entries=packed " in explain(**a)
    assert "form=wide-bits " in explain(**b) and " entries=cv " in explain(**b)


def test_accept_table_edge_moves():
    """table_scale * csr_row_abs_max = 2048 | 2049 with table_m = 2048 on both sides: the last table entry k = table_m is
    proposed in both runs, k = table_m + 1 in the second only, nothing beyond."""
    for name, L in (("t2048", 2048), ("t2049", 2049)):
        c = re_.csr_case(name)
        t = re_.csr_traits(c["csr"], c["h"])
        assert t["table_m"] == 2048 and t["acc"] == 0 and t["max_row_len"] <= 256   # (the several-updates-per-step rows form)
        m = (np.abs(c["J"]).astype(np.float64).sum(1) + np.abs(c["h"])).max()
        assert m == L and (m <= t["table_m"]) == (L == 2048)                         # sga_engine.cpp: table_covers
        ref, dE, s = re_.proposals(c["J"], c["h"], c["s0"], c["temps"], c["sweeps"], c["seed"])
        k = np.abs(dE) / 2.0
        assert (k == 2048).any() and (k == 2049).any() == (L == 2049) and k.max() == L
        assert (k[ref["accept_trace"].astype(bool)] > 1024).any()                    # large moves are taken, too


def test_fixed_point_twins_by_the_codes_condition():
    assert re_.fixed_point_bits(re_.FX_IN) == 32 and re_.fixed_point_bits(re_.FX_OUT) == 64
    assert re_.FX_OUT == re_.FX_IN + 1 and re_.FX_OUT < 2 ** 31   # (the plain bound 2^k B < 2^31 would admit both)
    for name, M, bits in (("fx_in", re_.FX_IN, 32), ("fx_out", re_.FX_OUT, 64)):
        c = re_.dense_case(name)
        a = np.abs(c["J"]).astype(np.float64) * 256.0
        assert np.array_equal(a, np.rint(a)) and (a % 2 == 1).any()           # multiples of 2^-8, k = 8
        rs = a.sum(1)
        assert rs[0] == M and (rs[1:] < M).all() and not c["h"].any()
        for csr in (False, True):
            t = re_.fixed_point_traits(c["J"], csr)
            assert t["clf_bits"] == bits
            assert f"fields=int{bits} fixed-point)" in explain(R_local=5, field_cache=1, **t)
        ref = re_.reference(name)
        acc = ref["accept_trace"].astype(bool)
        assert not acc[0].any() and acc[4].all() and np.array_equal(ref["spins"][0], c["xi"])   # +M held at T = 0
        assert all(acc[r].any() and not acc[r].all() for r in (1, 2, 3))
        assert np.array_equal(re_.reference(name, as_csr=True)["spins"], ref["spins"])
