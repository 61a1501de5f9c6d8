"""Shared-coupling batches (sga_set_dense_shared: one J, many field vectors) without a GPU: the version and the header,
the form selection's answers for hand-filled queries with `shared_j`, unchanged answers without it (two records of
tests/golden/route_table.json), and the pure grouping function behind BatchConfig(shared_couplings=True)."""
import json
import os
import re

import numpy as np
import pytest
import torch

import spin_glass_anneal_rl_amd as sg
from spin_glass_anneal_rl_amd import _native as N
from spin_glass_anneal_rl_amd import batch as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF, ON, AUTO = 0, 1, 2  # SGA_FIELD_CACHE_*


def int_query(n=300, R=12, storage=None, cache=OFF, n_models=3, shared_j=1, **kw):
    """Dense integer traits (table_m > 0, clf_ok, acc = 0) as an engine poses them."""
    storage = N.J_I8 if storage is None else storage
    elem = 1 if storage in (N.J_I8, N.J_T2) else 4
    ldj = (n * elem + 127) // 128 * 128 // elem
    fields = dict(kind=N.ROUTE_DENSE, n=n, n_models=n_models, shared_j=shared_j, R_local=R, storage=storage, acc=0, table_m=20,
                  clf_ok=1, clf_bits=16, clf_scale=1, field_cache=cache, sstride=ldj, ldj=ldj)
    fields.update(kw)
    return N.route_query(**fields)


def cached(q):
    return N.explain_route(q).split(" cached=")[1]


def test_version_header_and_binding():
    assert N.lib().sga_version() >= 1600
    text = open(os.path.join(ROOT, "include", "sga.h")).read()
    doc = re.search(r"/\* A batch with ONE coupling matrix.*?\*/\s*int sga_set_dense_shared\(", text, re.S)
    assert doc, "sga_set_dense_shared is documented in the header"
    for word in ("sga_set_dense_batch", "shared-J models=M", "sga_problem_checksum", "row-shared windows", "SGA_J_T2"):
        assert word in doc.group(0), word
    assert hasattr(N.lib(), "sga_set_dense_shared")
    # the query field took the place of a reserved word: same size, same offset, zeroed by the init call
    assert N.RouteQuery.shared_j.offset == N.RouteQuery.sstride.offset + 4 and N.RouteQuery.shared_j.size == 4
    assert N.RouteQuery.ldj.offset == N.RouteQuery.shared_j.offset + 4
    assert N.route_query().shared_j == 0


def test_row_shared_windows_open_to_shared_batches_only():
    forced = {"row_shared": 1}
    line = N.explain_route(int_query(options=forced))
    assert "sweep=row-shared" in line and "shared-J models=3" in line, line
    stacked = N.explain_route(int_query(shared_j=0, options=forced))
    assert "sweep=row-shared" not in stacked and "shared-J" not in stacked, stacked
    # ... and the stacked answer is the one-letter-for-letter answer it always was: nothing but the two additions differs
    assert line.replace(" shared-J models=3", "").replace(" sweep=row-shared(W=1024)", "") == stacked
    # the form's other conditions hold batch-wide: field cache OFF, an accept table, exact fp32 sums, the option
    assert "sweep=row-shared" not in N.explain_route(int_query(cache=ON, options=forced))
    assert "sweep=row-shared" not in N.explain_route(int_query(table_m=0, options=forced))
    assert "sweep=row-shared" not in N.explain_route(int_query(clf_ok=0, options=forced))
    assert "sweep=row-shared" not in N.explain_route(int_query(storage=N.J_F32, acc=1, options=forced))
    assert "sweep=row-shared" not in N.explain_route(int_query(options={"row_shared": 0}))
    # bit-plane storage is a shared batch's to have
    assert N.explain_route(int_query(storage=N.J_T2, options=forced)).startswith("dense storage=t2 ")


def _golden_dense_one_model(count):
    with open(os.path.join(ROOT, "tests", "golden", "route_table.json")) as f:
        cases = json.load(f)["cases"]
    picked = [c for c in cases if c["query"]["kind"] == N.ROUTE_DENSE and c["query"]["n_models"] == 1]
    assert len(picked) >= count
    return picked[:count]


@pytest.mark.parametrize("case", _golden_dense_one_model(2), ids=lambda c: c["name"][:24])
def test_answers_without_the_field_are_byte_identical(case):
    """shared_j = 0, one model: the line recorded from engines before the field existed."""
    q = N.route_query(**case["query"])
    assert q.shared_j == 0 and q.n_models == 1
    assert N.explain_route(q) == case["explain"]
    # one model is one matrix whatever the flag says: nothing is named, nothing is rerouted
    q.shared_j = 1
    assert N.explain_route(q) == case["explain"]


def test_cached_wording_names_the_batch():
    # ON / AUTO over integer couplings: as for a stacked batch
    for shared in (1, 0):
        on = cached(int_query(cache=ON, shared_j=shared))
        assert on.startswith("on(") and "models=3" in on and "fields=int16" in on, on
        auto = cached(int_query(cache=AUTO, shared_j=shared))
        assert auto.startswith("auto(") and "models=3" in auto, auto
    assert cached(int_query(cache=ON)) == cached(int_query(cache=ON, shared_j=0))
    assert cached(int_query(cache=AUTO)) == cached(int_query(cache=AUTO, shared_j=0))
    # the fixed-point form behind the two options a stacked batch needs
    fx = dict(storage=N.J_F32, acc=1, table_m=0, clf_ok=0, clf_bits=32)
    both = {"clf_fixed_point": 1, "batch_fixed_point": 1}
    on = cached(int_query(cache=ON, options=both, **fx))
    assert on == cached(int_query(cache=ON, shared_j=0, options=both, **fx))
    assert on.startswith("on(") and "fixed-point models=3" in on and "fields=int32" in on, on
    auto = cached(int_query(cache=AUTO, options=both, **fx))
    assert auto.startswith("auto(") and "models=3" in auto, auto
    # without "batch_fixed_point" the set-time scan refuses the form (clf_bits = 0), shared or not
    one = {"clf_fixed_point": 1}
    assert cached(int_query(cache=ON, options=one, **{**fx, "clf_bits": 0})) == "refused"
    assert cached(int_query(cache=AUTO, options=one, **{**fx, "clf_bits": 0})) == "unavailable"


# ----------------------------------------------------------------------------- BatchConfig(shared_couplings=True)
def _dense_model(J, h=None):
    n = J.shape[0]
    m = sg.IsingModel(sg.IsingModelConfig(n_spins=n, use_sparse=False))
    m.set_couplings_from_matrix(J)
    if h is not None:
        m.set_external_fields(torch.as_tensor(h, dtype=torch.float32))
    return m


def _sym(rng, n):
    J = np.triu(rng.randint(0, 2, (n, n)) * 2 - 1, 1).astype(np.float32)
    return torch.from_numpy(J + J.T)


class _Stub:
    """What shared_coupling_runs reads of a model: its couplings."""

    def __init__(self, couplings):
        self.couplings = couplings


def test_shared_coupling_runs():
    rng = np.random.RandomState(3)
    Ja, Jb = _sym(rng, 12), _sym(rng, 12)
    assert not torch.equal(Ja, Jb)
    runs = B.shared_coupling_runs
    # the same object -> one run
    assert runs([_Stub(Ja)] * 4) == [(0, 4)]
    # a view of the same storage with the same shape and strides -> one run
    assert runs([_Stub(Ja), _Stub(Ja.view(12, 12)), _Stub(Ja[:])]) == [(0, 3)]
    # equal content in different tensors -> one run
    assert runs([_Stub(Ja), _Stub(Ja.clone()), _Stub(Ja.clone())]) == [(0, 3)]
    # a differing J in the middle splits the runs
    assert runs([_Stub(Ja), _Stub(Ja), _Stub(Jb), _Stub(Ja), _Stub(Ja.clone())]) == [(0, 2), (3, 5)]
    # a sparse model ends a run
    sp = Ja.to_sparse()
    assert runs([_Stub(Ja), _Stub(Ja), _Stub(sp), _Stub(Ja)]) == [(0, 2)]
    assert runs([_Stub(sp), _Stub(sp)]) == []
    # a run of one is not shared
    assert runs([_Stub(Ja)]) == [] and runs([_Stub(Ja), _Stub(Jb), _Stub(Ja)]) == [] and runs([]) == []
    # another shape is another matrix
    assert runs([_Stub(Ja), _Stub(_sym(rng, 10))]) == []
    # real models, as BatchProcessor holds them
    models = [_dense_model(Ja, rng.randint(-1, 2, 12)) for _ in range(3)] + [_dense_model(Jb)]
    assert runs(models) == [(0, 3)]


def test_batch_config_flag_is_opt_in_and_routes_runs(monkeypatch):
    """No device: a stand-in engine records which setter each segment of a chunk goes through."""
    assert B.BatchConfig().shared_couplings is False
    with pytest.raises(ValueError):
        B.BatchConfig(shared_couplings=1)
    calls = []

    class Recorder:
        def __init__(self, device=0):
            self.R = 0

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def set_field_cache(self, mode="on"):
            pass

        def set_dense_batch(self, J, h, storage="auto"):
            calls.append(("set_dense_batch", J.shape, h.shape))
            self.n = J.shape[-1]

        def set_dense_shared(self, J, H, storage="auto"):
            calls.append(("set_dense_shared", J.shape, H.shape))
            self.n = J.shape[-1]

        def describe(self):
            return "dense n=12 shared-J models=2"

        def init_replicas(self, R, seed=0, s0=None):
            self.R = R

        def energies(self):
            return np.zeros(self.R)

        def sweep(self, n_sweeps=1, sched=None):
            pass

        def stats(self):
            return np.zeros(self.R, np.int64), np.ones(self.R, np.int64)

        def best(self, r):
            return 0.0, np.ones(self.n, np.int8), 0

    monkeypatch.setattr(B, "AnnealEngine", Recorder)
    rng = np.random.RandomState(5)
    Ja, Jb = _sym(rng, 12), _sym(rng, 12)
    models = [_dense_model(Ja), _dense_model(Ja), _dense_model(Jb), _dense_model(Jb.clone()), _dense_model(_sym(rng, 12))]
    cfg = sg.GPUAnnealerConfig(n_sweeps=10, random_seed=1)
    out = B.BatchProcessor(cfg, B.BatchConfig()).process_models_batch(models)
    assert len(out) == 5 and calls == [("set_dense_batch", (5, 12, 12), (5, 12))]
    calls.clear()
    bp = B.BatchProcessor(cfg, B.BatchConfig(shared_couplings=True))
    out = bp.process_models_batch(models)
    assert len(out) == 5 and all(r is not None for r in out)
    assert calls == [("set_dense_shared", (12, 12), (2, 12)), ("set_dense_shared", (12, 12), (2, 12)),
                     ("set_dense_batch", (1, 12, 12), (1, 12))], calls
    assert "shared-J" in bp.last_description
