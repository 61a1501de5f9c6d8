"""Group couplings plus a stored sparse remainder (sga_set_groups_csr), the parts that need no GPU: the binding, the
encoders' groups + remainder against the assembled couplings, the route strings, and the CONDITIONS ON THE INPUTS of
tests/test_groups_rest_gpu.py -- checked on the oracle's traced runs of the same problems, so that the GPU comparison
is known to walk through the production kernel's remainder fix-up (an accept at a site a, then a still-undecided
candidate i of the same window with R_ia != 0; on the big instance also across two waves of one super-window)."""
import numpy as np
import pytest

import groups_rest_cases as grc


def test_version_and_symbol():
    from spin_glass_anneal_rl_amd import _native as N
    assert N.lib().sga_version() >= 1200
    assert hasattr(N.lib(), "sga_set_groups_csr")
    assert N.GROUPS_MAX_REST_ROW == grc.MAX_REST_ROW


def _same_csr(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("which", ["scheduling_precedence", "qubo_pair"])
def test_group_rest_structure_materialises_to_the_assembled_couplings(which):
    from spin_glass_anneal_rl_amd import encoders as E
    if which == "scheduling_precedence":
        args = ([1, 2, 1], 1, 6, 6)
        w = {"assignment": 4, "capacity": 2, "precedence": 4}
        b = E.scheduling_ising(*args, penalty_weights=w)
        wrapped = E.scheduling_groups_rest(*args, w)
    else:
        b = E.assignment_ising(4, 5, weight=8.0)
        b.add_qubo_pair([0, 3, 7], [6, 19, 8], [2.0, -4.0, 1.0])  # (7, 8) share a group: J accumulates across the parts
        b.add_coupling([1], [2], [0.5])
        b.add_coupling([1], [2], [-0.5])                            # ... and an exact zero, dropped
        wrapped = None
    mp, mem, coeff, rest, h, const = b.group_rest_structure()
    assert mp.dtype == np.int64 and mem.dtype == np.int32 and coeff.dtype == np.float32 and h.dtype == np.float32
    assert rest[0].dtype == np.int32 and rest[1].dtype == np.int32 and rest[2].dtype == np.float32
    assert rest[1].size > 0 and (rest[2] != 0).all()
    assert _same_csr(grc.materialise(b.n, mp, mem, coeff, rest), b.to_csr())
    assert np.array_equal(h, b.fields()) and const == b.constant
    with pytest.raises(ValueError, match="add_cardinality_groups"):  # (what tests/test_groups_host.py pins stays)
        b.group_structure()
    if wrapped is not None:
        assert wrapped[0] == b.n and _same_csr(wrapped[4], rest)
        assert all(np.array_equal(x, y) for x, y in zip(wrapped[1:4] + wrapped[5:6], (mp, mem, coeff, h)))
        with pytest.raises(ValueError, match="precedence"):
            E.scheduling_groups(*args, penalty_weights=w)


def test_group_rest_structure_without_other_couplings_and_refusals():
    from spin_glass_anneal_rl_amd import encoders as E
    b = E.assignment_ising(3, 3)
    mp, mem, coeff, rest, h, const = b.group_rest_structure()
    assert rest[1].size == 0 and np.array_equal(rest[0], np.zeros(10, np.int32))
    assert all(np.array_equal(x, y) for x, y in zip((mp, mem, coeff, h), b.group_structure()[:4]))
    with pytest.raises(ValueError, match="physical"):
        E.assignment_ising(3, 3, convention="reference").group_rest_structure()


def test_precedence_pairs_default_is_every_pair():
    from spin_glass_anneal_rl_amd import encoders as E
    args = ([1.0, 2.0, 1.0, 2.0], 2, 6, 6)
    a = E.scheduling_ising(*args)
    b = E.scheduling_ising(*args, precedence_pairs=None)
    c = E.scheduling_ising(*args, precedence_pairs=[(i, j) for i in range(4) for j in range(i + 1, 4)])
    for x in (b, c):
        assert _same_csr(a.to_csr(), x.to_csr()) and np.array_equal(a.fields(), x.fields()) and a.constant == x.constant
    chain = E.scheduling_ising(*args, precedence_pairs=[(0, 1), (1, 2), (2, 3)])
    assert chain.to_csr()[1].size < a.to_csr()[1].size
    with pytest.raises(ValueError, match="precedence_pairs"):
        E.scheduling_ising(*args, precedence_pairs=[(0, 4)])


def test_route_names_the_remainder():
    from spin_glass_anneal_rl_amd import _native as N
    base = dict(kind=N.ROUTE_GROUPS, n=50000, n_groups=600, group_max=100, R_local=1024)
    plain = N.explain_route(N.route_query(**base))
    assert "rest_" not in plain
    assert N.explain_route(N.route_query(rest_nnz=0, rest_max_row=0, **base)) == plain
    line = N.explain_route(N.route_query(rest_nnz=9900000, rest_max_row=200, **base))
    head, tail = plain.split(" cached=")
    assert line == head + " rest_nnz=9900000 rest_max_row=200 cached=" + tail
    # a remainder without groups is a legal query, nothing at all is not
    assert "rest_nnz=80" in N.explain_route(N.route_query(kind=N.ROUTE_GROUPS, n=40, n_groups=0, rest_nnz=80, rest_max_row=3))
    with pytest.raises(N.AnnealingError):
        N.explain_route(N.route_query(kind=N.ROUTE_GROUPS, n=40, n_groups=0))


@pytest.mark.parametrize("name", grc.NAMES)
def test_instances_are_in_the_exact_class_and_within_the_row_limit(name):
    n, mp, mem, c, rest, h, csr = grc.problem(name)
    coupling = c[np.diff(mp) >= 2]  # (a singleton group adds no coupling, whatever its coefficient)
    assert np.abs(coupling).max(initial=0) <= 4 and np.abs(rest[2]).max() <= 2
    assert np.diff(rest[0]).max() <= grc.MAX_REST_ROW
    assert np.array_equal(c * 2, np.round(c * 2)) and np.array_equal(rest[2] * 2, np.round(rest[2] * 2))  # grid 2^-1
    assert 2 * np.add.reduceat(np.abs(np.r_[csr[2], 0.0]), np.minimum(csr[0][:-1], csr[2].size)).max() < 2 ** 24


@pytest.mark.parametrize("name", grc.NAMES)
def test_input_conditions_accepts_and_refusals(name):
    n = grc.problem(name)[0]
    tr = grc.oracle_traced(name)
    acc, dE = tr["accept"].astype(bool), tr["dE"]
    assert 0 < acc[0].sum() < acc[0].size            # the hottest replica accepts some proposals and refuses some
    # the coldest refuses an uphill proposal: fewer accepts than proposals, and at T = 0.1 on the 2^-1 grid a refused
    # proposal is uphill (dE <= 0 is always accepted)
    assert acc[-1].sum() < acc[-1].size
    assert (dE[-1][~acc[-1]] == 0).all()


@pytest.mark.parametrize("name", grc.FIXUP_NAMES)
def test_input_conditions_the_fix_up_is_exercised(name):
    assert grc.fixup_events(name) > 0
    if name == "big_n700_rest":  # ... and from one wave's 128 updates to the next wave's, at 2 waves per replica
        assert grc.fixup_events(name, span=2 * grc.WINDOW, across=grc.WINDOW) > 0
