"""Option "clf_fixed_point" without a GPU: the option is listed and documented, the form selection's answer for
hand-filled CSR queries (fixed-point widths, LDS limits, refusals), and the public classes' flag."""
import dataclasses
import inspect
import os
import re

import pytest

from spin_glass_anneal_rl_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_is_listed_documented_and_off_by_default():
    names = N.option_names()
    assert "clf_fixed_point" in names
    q = N.route_query(kind=N.ROUTE_CSR, n=100)
    assert q.opt[names.index("clf_fixed_point")] == 0
    text = open(os.path.join(ROOT, "include", "sga.h")).read()
    doc = re.search(r"/\* Form-selection options of ONE engine.*?\*/", text, re.S).group(0)
    entry = re.search(r'^ \*   "clf_fixed_point"(.*?)(?=^ \*   "|\Z)', doc, re.S | re.M).group(1)
    assert "0 (default) | 1" in entry and "[set]" in entry
    assert N.lib().sga_version() >= 700


def c5_query(n_cities=100, R=2048, **kw):
    """What an engine poses for the TSP QUBO of encoders.tsp_csr (real-valued distances: acc class f64-exact)."""
    n = n_cities * n_cities
    deg = 4 * (n_cities - 1)
    fields = dict(kind=N.ROUTE_CSR, n=n, R_local=R, nnz=n * deg, max_row_len=deg, layout_entries=n * deg, acc=2,
                  table_m=0, clf_ok=1, clf_bits=64, field_cache=1)
    fields.update(kw)
    return N.route_query(**fields)


ON, AUTO = 1, 2  # SGA_FIELD_CACHE_ON, SGA_FIELD_CACHE_AUTO


def test_fixed_point_queries_get_the_new_answers():
    out = N.explain_route(c5_query(options={"clf_fixed_point": 1}))
    assert out.endswith(" cached=on(waves=8 fields=int64 fixed-point)"), out
    out = N.explain_route(c5_query(clf_bits=32, n_cities=40, options={"clf_fixed_point": 1}))
    assert out.endswith(" cached=on(waves=4 fields=int32 fixed-point)"), out
    # short rows, few spins: four waves
    q = N.route_query(kind=N.ROUTE_CSR, n=3000, R_local=8, nnz=3000 * 12, max_row_len=20, layout_entries=3000 * 12,
                      acc=2, clf_ok=1, clf_bits=32, field_cache=ON, options={"clf_fixed_point": 1})
    assert N.explain_route(q).endswith(" cached=on(waves=4 fields=int32 fixed-point)"), N.explain_route(q)


def test_without_the_option_the_answers_are_todays():
    # the query an engine poses for a real-valued problem with the option off: clf_ok = 0, clf_bits = 16
    for cache, word in ((ON, "refused"), (AUTO, "unavailable")):
        out = N.explain_route(c5_query(clf_ok=0, clf_bits=16, field_cache=cache))
        assert out.endswith(f" cached={word}"), out
    # an int16 problem: the option changes nothing (the engine keeps the int16 form and reports clf_bits = 16)
    q = dict(kind=N.ROUTE_CSR, n=5000, R_local=16, nnz=5000 * 12, max_row_len=20, layout_entries=5000 * 12, acc=0,
             table_m=30, clf_ok=1, field_cache=ON)
    a = N.explain_route(N.route_query(**q))
    b = N.explain_route(N.route_query(**q, options={"clf_fixed_point": 1}))
    assert a == b and a.endswith(" cached=on(waves=4)"), (a, b)
    q["field_cache"] = AUTO
    assert N.explain_route(N.route_query(**q)) == N.explain_route(N.route_query(**q, options={"clf_fixed_point": 1}))


def test_lds_refusal_at_the_right_size():
    def cached(n, bits):
        q = N.route_query(kind=N.ROUTE_CSR, n=n, R_local=4, nnz=n * 8, max_row_len=8, layout_entries=n * 8, acc=2,
                          clf_ok=1, clf_bits=bits, field_cache=ON, options={"clf_fixed_point": 1})
        return N.explain_route(q).split(" cached=")[1]
    # int64: 8 bytes per spin + its bit: about 20 000 spins per replica in 160 KiB
    assert cached(19000, 64).startswith("on(") and cached(21000, 64) == "refused"
    assert cached(39000, 32).startswith("on(") and cached(40000, 32) == "refused"
    # C5 at 1000 cities: 10^6 fields do not fit (nor do its rows of 3996 entries)
    assert N.explain_route(c5_query(n_cities=1000, R=64, options={"clf_fixed_point": 1})).endswith(" cached=refused")


def test_refusals_with_the_option_on():
    # rows longer than 2048 entries
    q = N.route_query(kind=N.ROUTE_CSR, n=5000, R_local=4, nnz=5000 * 2100, max_row_len=2100, layout_entries=5000 * 2112,
                      slotted=1, acc=2, clf_ok=1, clf_bits=32, field_cache=ON, options={"clf_fixed_point": 1})
    assert N.explain_route(q).endswith(" cached=refused")
    # the canonical accumulation class: no exact fixed point
    q = N.route_query(kind=N.ROUTE_CSR, n=500, R_local=4, nnz=5000, max_row_len=10, layout_entries=5000, acc=3,
                      clf_ok=0, clf_bits=16, field_cache=ON, options={"clf_fixed_point": 1})
    assert N.explain_route(q).endswith(" cached=refused")
    # ragged batches and the implicit TSP form stay refused
    q = N.route_query(kind=N.ROUTE_CSR, n=100, n_models=3, nnz=300, max_row_len=3, layout_entries=300, acc=2, clf_ok=1,
                      clf_bits=32, field_cache=ON, options={"clf_fixed_point": 1})
    assert N.explain_route(q).endswith(" cached=refused")
    q = N.route_query(kind=N.ROUTE_TSP, n=400, n_cities=20, field_cache=ON, options={"clf_fixed_point": 1})
    assert N.explain_route(q).endswith(" cached=refused")


def test_auto_break_even_accounts_for_width_and_exp_path():
    def theta(bits, opt):
        q = c5_query(field_cache=AUTO, clf_bits=bits, options={"clf_fixed_point": opt})
        out = N.explain_route(q)
        m = re.search(r"cached=auto\(start=(\w+) theta=([0-9.]+)\)", out)
        assert m, out
        assert m.group(1) == "rows"   # CSR: a run starts on the row kernels
        return float(m.group(2))
    t64, t32, t16 = theta(64, 1), theta(32, 1), theta(16, 1)
    assert t64 < t32 < t16
    assert theta(16, 0) == t16   # the int16 form's break-even is unchanged


def test_public_classes_take_the_flag_and_default_to_off():
    import spin_glass_anneal_rl_amd as sg
    from spin_glass_anneal_rl_amd.scheduler import SpinGlassScheduler
    for cls in (sg.GPUAnnealerConfig, sg.ParallelTemperingConfig):
        f = {x.name: x for x in dataclasses.fields(cls)}
        assert f["fixed_point_fields"].default is False, cls
    assert sg.GPUAnnealerConfig(n_sweeps=3, fixed_point_fields=True).fixed_point_fields is True
    assert sg.ParallelTemperingConfig(n_sweeps=3, fixed_point_fields=True).fixed_point_fields is True
    p = inspect.signature(SpinGlassScheduler.anneal).parameters["fixed_point_fields"]
    assert p.default is False
