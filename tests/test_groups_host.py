"""Implicit cardinality-group couplings (sga_set_groups), the parts that need no GPU: the encoders' group structure
against the assembled couplings, the C ABI's version and route answers, and the CONDITIONS ON THE INPUTS of
tests/test_groups_gpu.py -- checked here on the oracle's traced runs of the same problems, so that the GPU comparison
is known to walk through every branch of the window kernel (two accepts of one window sharing a group, a site proposed
again behind its own accept, a window without accept)."""
import json
import os

import numpy as np
import pytest

import groups_cases as gc


def _csr_of(builder):
    rp, ci, v = builder.to_csr()
    return rp, ci, v


@pytest.mark.parametrize("which", ["assignment", "scheduling"])
def test_group_structure_materialises_to_the_assembled_couplings(which):
    from spin_glass_anneal_rl_amd import encoders as E
    if which == "assignment":
        b = E.assignment_ising(5, 7)
        wrapped = E.assignment_groups(5, 7)
    else:
        args = ([1.0, 2.0, 2.0, 1.0], 2, 6, 6)  # durations of one and two slots
        w = {"assignment": 100.0, "capacity": 50.0}
        b = E.scheduling_ising(*args, penalty_weights=w)
        wrapped = E.scheduling_groups(*args, penalty_weights=w)
    mp, mem, coeff, h, const = b.group_structure()
    assert mp.dtype == np.int64 and mem.dtype == np.int32 and coeff.dtype == np.float32 and h.dtype == np.float32
    rp, ci, v = gc.materialise(b.n, mp, mem, coeff)
    rp0, ci0, v0 = _csr_of(b)
    assert np.array_equal(rp, rp0) and np.array_equal(ci, ci0) and np.array_equal(v, v0)
    assert np.array_equal(h, b.fields()) and const == b.constant
    assert wrapped[0] == b.n and all(np.array_equal(x, y) for x, y in zip(wrapped[1:5], (mp, mem, coeff, h)))
    if which == "scheduling":  # pairs that lie in two capacity groups: J accumulates
        assert (np.abs(v) > 25.0).any() and (np.abs(v) == 25.0).any()


def test_group_structure_refuses_what_is_no_group_sum():
    from spin_glass_anneal_rl_amd import encoders as E
    b = E.assignment_ising(3, 3)
    b.add_qubo_pair([0], [4], [1.0])
    with pytest.raises(ValueError, match="add_cardinality_groups"):
        b.group_structure()
    b = E.assignment_ising(3, 3)
    b.add_coupling([0], [1], [1.0])
    with pytest.raises(ValueError):
        b.group_structure()
    b = E.IsingBuilder(6)
    b.add_equality([0, 1, 2], [1.0, 2.0, 1.0], 1.0)
    with pytest.raises(ValueError):
        b.group_structure()
    with pytest.raises(ValueError, match="physical"):
        E.assignment_ising(3, 3, convention="reference").group_structure()
    b = E.IsingBuilder(9, "physical", overwrite=True)
    b.add_cardinality_groups(np.arange(9).reshape(3, 3), 1, 2.0)
    with pytest.raises(ValueError, match="overwrite"):
        b.group_structure()
    with pytest.raises(ValueError, match="precedence"):
        E.scheduling_groups([1.0, 2.0], 1, 4, 4, penalty_weights={"assignment": 4.0, "capacity": 2.0, "precedence": 1.0})


def test_version_and_symbol():
    from spin_glass_anneal_rl_amd import _native as N
    assert N.lib().sga_version() >= 1000
    assert hasattr(N.lib(), "sga_set_groups")


def test_route_names_the_groups_form():
    from spin_glass_anneal_rl_amd import _native as N
    # C4 as groups: 50 000 spins, 600 groups, 1024 replicas on 256 CUs
    q = N.route_query(kind=N.ROUTE_GROUPS, n=50000, n_groups=600, group_max=100, R_local=1024)
    line = N.explain_route(q)
    assert line.startswith("groups n_groups=600 ") and "sums=int16" in line and "waves=4 " in line
    assert "kernel=sweep_groups_kernel|sweep_groups_general_kernel" in line and line.endswith(" cached=off")
    assert "waves=2 " in N.explain_route(N.route_query(kind=N.ROUTE_GROUPS, n=50000, n_groups=600, group_max=100, R_local=1024,
                                                       tune_waves=2))
    assert "sums=int32" in N.explain_route(N.route_query(kind=N.ROUTE_GROUPS, n=10 ** 5, n_groups=2, group_max=1 << 15))
    general = N.explain_route(N.route_query(kind=N.ROUTE_GROUPS, n=299, n_groups=36, group_max=23, options={"force_general": 1}))
    assert general.split("kernel=")[1].split()[0] == "sweep_groups_general_kernel"
    assert "cached=refused" in N.explain_route(N.route_query(kind=N.ROUTE_GROUPS, n=299, n_groups=36, group_max=23, field_cache=1))
    assert "cached=unavailable" in N.explain_route(N.route_query(kind=N.ROUTE_GROUPS, n=299, n_groups=36, group_max=23, field_cache=2))
    assert N.explain_route(N.route_query(kind=N.ROUTE_GROUPS, n=2 * 10 ** 6, n_groups=10, group_max=10)).startswith("groups error=")
    with pytest.raises(Exception):
        N.explain_route(N.route_query(kind=N.ROUTE_GROUPS, n=10))  # no groups


def test_existing_route_answers_are_unchanged():
    from spin_glass_anneal_rl_amd import _native as N
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "route_table.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) >= 25
    for c in cases:
        assert N.explain_route(N.route_query(**c["query"])) == c["explain"], c["name"]


def test_option_documentation_stays_in_step():
    import test_host_logic
    test_host_logic.test_engine_options_are_documented_and_the_environment_is_read_in_one_place()


# ---------------------------------------------------------------------------------------------------------------------
# conditions on the inputs of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def _windows(name):
    """Per (replica, sweep, window): the proposed sites and accept flags of its <= 128 updates, in chain order."""
    n = gc.problem(name)[0]
    tr = gc.oracle_traced(name)
    R = tr["accept"].shape[0]
    for r in range(R):
        for k in range(gc.SWEEPS):
            for w0 in range(0, n, gc.WINDOW):
                sl = slice(k * n + w0, k * n + min(n, w0 + gc.WINDOW))
                yield tr["sites"][r, sl], tr["accept"][r, sl].astype(bool)


@pytest.mark.parametrize("name", gc.NAMES)
def test_production_runs_walk_every_branch_of_the_window_kernel(name):
    groups = gc.site_groups(name)
    shared = again = empty = False
    for sites, acc in _windows(name):
        hit = [int(s) for s in sites[acc]]
        empty = empty or not hit
        for a in range(len(hit)):
            for b in range(a + 1, len(hit)):
                shared = shared or (hit[a] != hit[b] and bool(groups[hit[a]] & groups[hit[b]]))
        for t in np.nonzero(acc)[0]:
            again = again or int(sites[t]) in [int(s) for s in sites[t + 1:]]
    assert shared, "no window with two accepted updates that share a group"
    assert again, "no window in which a site is proposed again after its own accept"
    assert empty, "no window without an accept"
    tr = gc.oracle_traced(name)
    assert 0 < tr["n_accepted"].sum() < tr["accept"].size  # the run accepts neither everything nor nothing


def test_big_instance_has_the_features_the_gpu_test_names():
    n, mp, mem, c, h, csr = gc.problem("big_n700")
    sizes = np.diff(mp)
    assert n % gc.WINDOW != 0 and n > 4 * gc.WINDOW          # a partial last window; two super-windows at four waves
    assert sizes.max() == 300 and (sizes == 1).any() and len(set(c.tolist())) >= 2
    assert not gc.site_groups("big_n700")[699]               # a site in no group
    assert (np.abs(h * 2 % 2) == 1).any() and np.array_equal(h * 2, np.round(h * 2))
    # K_i varies on the scheduling instance
    k = [len(g) for g in gc.site_groups("scheduling_6x1x12")]
    assert min(k) == 2 and max(k) == 4
