"""Cached local fields for ragged CSR batches without a GPU: the option, the version, the route answers for hand-filled
queries, and the condition on the test batches (every model is both accepted and rejected in)."""
import os
import re

import numpy as np

import ragged_clf_cases as rc
from spin_glass_anneal_rl_amd import _native as N
from spin_glass_anneal_rl_amd.batch import BatchConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ragged_query(**kw):
    base = dict(kind=N.ROUTE_CSR, n=1201, n_models=6, R_local=18, nnz=30906, max_row_len=95, layout_entries=30906, acc=0,
                table_m=196, table_scale=2, sstride=1216)
    opts = kw.pop("options", None)
    return N.route_query(**{**base, **kw, **({"options": opts} if opts else {})})


def test_option_exists_defaults_to_off_and_is_documented():
    names = N.option_names()
    assert names[-1] == "ragged_field_cache"  # appended: recorded route queries keep their indices
    q = N.route_query(kind=N.ROUTE_CSR, n=10)
    assert q.opt[names.index("ragged_field_cache")] == 0
    text = open(os.path.join(ROOT, "include", "sga.h")).read()
    doc = re.search(r"/\* Form-selection options of ONE engine.*?\*/", text, re.S).group(0)
    line = re.search(r'^ \*   "ragged_field_cache"\s+0 \(default\) \| 1.*?\[set\]', doc, re.M | re.S)
    assert line, "include/sga.h does not document the option as 0 (default) | 1 [set]"
    assert BatchConfig().ragged_field_cache is False


def test_version():
    assert N.lib().sga_version() >= 1100


def test_route_of_a_ragged_query():
    on = {"ragged_field_cache": 1}
    # option 0: every existing answer
    assert N.explain_route(ragged_query(field_cache=1, clf_ok=1)).endswith(" cached=refused")
    assert N.explain_route(ragged_query(field_cache=2, clf_ok=1)).endswith(" cached=unavailable")
    assert N.explain_route(ragged_query(field_cache=0, clf_ok=1)).endswith(" cached=off")
    streaming = N.explain_route(ragged_query()).rsplit(" cached=", 1)[0]
    assert streaming.startswith("csr form=narrow ragged models=6 spins=int8 waves=1 ")
    # option 1
    out = N.explain_route(ragged_query(field_cache=1, clf_ok=1, options=on))
    assert out == streaming + " cached=on(waves=4 models=6)", out
    out = N.explain_route(ragged_query(field_cache=1, clf_ok=1, max_row_len=257, options=on))
    assert out.endswith(" cached=on(waves=8 models=6)"), out
    out = N.explain_route(ragged_query(field_cache=1, clf_ok=1, max_row_len=256, options=on))
    assert out.endswith(" cached=on(waves=4 models=6)"), out
    assert N.explain_route(ragged_query(field_cache=1, clf_ok=0, options=on)).endswith(" cached=refused")
    assert N.explain_route(ragged_query(field_cache=2, clf_ok=0, options=on)).endswith(" cached=unavailable")
    assert N.explain_route(ragged_query(field_cache=0, clf_ok=1, options=on)).endswith(" cached=off")
    out = N.explain_route(ragged_query(field_cache=2, clf_ok=1, options=on))
    assert re.search(r" cached=auto\(start=rows theta=0\.\d+ models=6\)$", out), out
    # a row past 2048 entries, and a largest model past LDS (int16 fields of 80 000 spins): refused
    assert N.explain_route(ragged_query(field_cache=1, clf_ok=1, max_row_len=2049, options=on)).endswith(" cached=refused")
    assert N.explain_route(ragged_query(field_cache=1, clf_ok=1, n=80000, sstride=80000, options=on)).endswith(" cached=refused")
    # a one-model CSR query does not read the option
    one = dict(kind=N.ROUTE_CSR, n=1201, R_local=18, nnz=9934, max_row_len=20, layout_entries=9934, acc=0, table_m=60,
               sstride=1216, field_cache=1, clf_ok=1)
    assert N.explain_route(N.route_query(**one)) == N.explain_route(N.route_query(**one, options=on))


def test_batches_walk_both_paths_in_every_model():
    for name, longest in (("S", (65, 256)), ("L", (513, 1024))):
        probs = rc.batch(name)
        lo, hi = longest
        assert lo <= rc.longest_row(probs) <= hi  # S: four waves, one entry per thread; L: eight waves, two per thread
        rates = rc.check_acceptance(name)
        assert len(rates) == len(probs)
    assert rc.sizes(rc.batch("S")) == [3, 37, 100, 257, 700, 1201]
    assert rc.sizes(rc.batch("L")) == [3, 37, 257, 1500]
    # the half-integer model makes the batch-wide scale 2; every other model's h is integer
    for name in "SL":
        halves = [bool(np.any(p[3] != np.rint(p[3]))) for p in rc.batch(name)]
        assert halves[1] and sum(halves) == 1
