"""Shared-coupling CSR batches (sga_set_csr_shared: one set of CSR rows, many field vectors) without a GPU: the version,
the header and the binding, the form selection's answers for hand-filled CSR queries with `shared_j` -- the one-model
decision among the one-wave-per-replica forms, each refusal's text, the ragged answers without the flag -- and the pure
grouping function behind BatchConfig(shared_couplings=True) for sparse chunks."""
import ctypes as C
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
CSR_STORAGE_PACKED = 2   # SGA_CSR_STORAGE_PACKED
REFUSAL = "csr error=shared-coupling CSR batches"


def csr_query(n=10000, degree=32, longest=None, R=4096, n_models=3, shared_j=1, **kw):
    """An integer CSR problem (accept-table class) as an engine poses it: `degree` entries per row on average, the
    longest row `longest` (default: the degree -- a regular graph), unpadded layout, 32-bit extents."""
    longest = degree if longest is None else longest
    fields = dict(kind=N.ROUTE_CSR, n=n, nnz=n * degree, max_row_len=longest, layout_entries=n * degree, acc=0,
                  table_m=longest + 1, table_scale=1, rowptr32=1, clf_ok=1, R_local=R, n_models=n_models, shared_j=shared_j)
    fields.update(kw)
    return N.route_query(**fields)


def word(line, key):
    m = re.search(r"\b%s=(\S+)" % re.escape(key), line)
    assert m, (key, line)
    return m.group(1)


def test_version_header_and_binding():
    assert N.lib().sga_version() >= 1700
    text = open(os.path.join(ROOT, "include", "sga.h")).read()
    decl = re.search(r"int sga_set_csr_shared\(([^;]*)\);", text, re.S)
    assert decl, "sga_set_csr_shared is declared in the header"
    args = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S)
    assert [re.sub(r"\s+", " ", a).strip() for a in args.split(",")] == [
        "sga_engine *e", "const int32_t *rowptr", "const int32_t *colidx", "const float *val", "const float *H", "int n",
        "int64_t nnz", "int n_models"]
    doc = re.search(r"/\* ONE set of CSR rows under n_models field vectors.*?\*/\s*int sga_set_csr_shared\(", text, re.S)
    assert doc, "sga_set_csr_shared is documented in the header"
    for w in ("shared-J models=M", "sga_problem_checksum", "shared-coupling CSR batches", "non-finite", "replica0",
              "sga_set_csr_batch", "n_models = 1 is sga_set_csr"):
        assert w in doc.group(0), w
    fn = N.lib().sga_set_csr_shared
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p] * 5 + [C.c_int, C.c_int64, C.c_int]
    assert "SGA_ROUTE_CSR" in re.search(r"int32_t shared_j;[^\n]*", text).group(0)
    assert hasattr(sg.AnnealEngine, "set_csr_shared")


def test_shared_queries_take_the_one_model_decision():
    # C3-like: 10 000 spins, degree 32, 4096 replicas -> several updates per step, eight rows of eight lanes
    line = N.explain_route(csr_query())
    assert line.startswith("csr form=rows ") and word(line, "updates_per_step") == "8" and " shared-J models=3" in line, line
    assert word(line, "waves") == "1" and word(line, "spins") == "int8" and word(line, "cached") == "off"
    # ... and it is the one-model line with the kind named, nothing else
    one = N.explain_route(csr_query(n_models=1))
    assert line.replace(" shared-J models=3", "") == one and "shared-J" not in one
    # degree 6 (a 3-D lattice) and degree 40: G = 8 and G = 4
    assert word(N.explain_route(csr_query(degree=6)), "updates_per_step") == "8"
    deg40 = N.explain_route(csr_query(degree=40))
    assert deg40.startswith("csr form=rows ") and word(deg40, "updates_per_step") == "4"
    # a longest row of 100: the medium rows build (four per step, 8 entries per lane), integer problems only
    medium = N.explain_route(csr_query(degree=40, longest=100))
    assert medium.startswith("csr form=rows ") and word(medium, "updates_per_step") == "4" and "shared-J models=3" in medium
    real = N.explain_route(csr_query(degree=40, longest=100, acc=3, table_m=0, clf_ok=0))
    assert real.startswith("csr form=narrow ") and word(real, "updates_per_step") == "0" and "shared-J models=3" in real
    # the options act as on one model: bit spins, the one-update form, the pair look-ahead
    bits = N.explain_route(csr_query(options={"force_csr_bits": 1}))
    assert bits.startswith("csr form=rows spins=bits ") and "shared-J models=3" in bits, bits
    assert N.explain_route(csr_query(options={"force_csr_bits": 1, "csr_updates_per_step": 0})).startswith("csr form=narrow-bits ")
    assert N.explain_route(csr_query(options={"csr_updates_per_step": 0})).startswith("csr form=narrow spins=int8 ")
    assert word(N.explain_route(csr_query(options={"csr_updates_per_step": 2})), "updates_per_step") == "2"
    for opts in ({"force_csr_bits": 1}, {"csr_updates_per_step": 0}, {"csr_updates_per_step": 2}):
        assert N.explain_route(csr_query(options=opts)).replace(" shared-J models=3", "") == \
            N.explain_route(csr_query(n_models=1, options=opts))
    # a long-row problem one model would deal to two waves runs narrow here, as a ragged batch does
    long_rows = dict(n=1000, degree=300, longest=400, R=512)
    assert N.explain_route(csr_query(n_models=1, **long_rows)).startswith("csr form=wide-bytes ")
    narrow = N.explain_route(csr_query(**long_rows))
    assert narrow.startswith("csr form=narrow spins=int8 waves=1 ") and "shared-J models=3" in narrow, narrow
    # AUTO streams
    assert word(N.explain_route(csr_query(field_cache=AUTO)), "cached") == "unavailable"


def test_the_golden_c3_query_shared():
    with open(os.path.join(ROOT, "tests", "golden", "route_table.json")) as f:
        c3 = [c for c in json.load(f)["cases"] if c["name"].startswith("BASELINE c3")][0]
    q = N.route_query(**c3["query"])
    assert N.explain_route(q) == c3["explain"]
    q.n_models, q.shared_j = 3, 1
    # (its longest row has 50 entries: four updates per step, as for one model)
    assert N.explain_route(q) == c3["explain"].replace(" cached=", " shared-J models=3 cached=")


@pytest.mark.parametrize("name, change, text", [
    ("tune_waves", dict(tune_waves=2), " run one wave per replica (sga_set_tuning waves_per_replica > 1"),
    ("too_large", dict(n=2_000_000, degree=6), ": the problem fits no one-wave-per-replica form"),
    ("field_cache_on", dict(field_cache=ON), ": cached local fields are not built for them"),
    ("packed", dict(storage=CSR_STORAGE_PACKED), " read (column, value) entries (packed storage"),
])
def test_refusals(name, change, text):
    line = N.explain_route(csr_query(**change))
    assert line.startswith(REFUSAL + text), line
    # one wave per replica asked for explicitly is what these batches run
    assert N.explain_route(csr_query(tune_waves=1)).startswith("csr form=rows ")


@pytest.mark.parametrize("change", [dict(), dict(degree=6), dict(degree=40, longest=100), dict(tune_waves=2),
                                    dict(field_cache=ON), dict(field_cache=AUTO), dict(storage=CSR_STORAGE_PACKED),
                                    dict(options={"force_csr_bits": 1}), dict(options={"csr_updates_per_step": 2})])
def test_without_the_flag_the_answers_are_the_ragged_ones(change):
    """shared_j = 0 with n_models = 3 is a ragged batch: the narrow one-update form or its refusals, as before."""
    line = N.explain_route(csr_query(shared_j=0, **change))
    assert "shared" not in line, line
    if change.get("tune_waves") or change.get("storage") or change.get("options"):
        assert line.startswith("csr error=ragged CSR batches "), line
    else:
        assert line.startswith("csr form=narrow ragged models=3 spins=int8 waves=1 ") and word(line, "updates_per_step") == "1", line
        assert word(line, "cached") == {OFF: "off", ON: "refused", AUTO: "unavailable"}[change.get("field_cache", OFF)]


# ----------------------------------------------------------------------------- BatchConfig(shared_couplings=True), sparse chunks
class _Stub:
    """What shared_sparse_runs reads of a model: its couplings and its size."""

    def __init__(self, couplings):
        self.couplings = couplings
        self.n_spins = couplings.shape[0]


def _sym(rng, n, p=0.4):
    J = np.triu((rng.rand(n, n) < p) * (rng.randint(0, 2, (n, n)) * 2 - 1), 1).astype(np.float32)
    return torch.from_numpy(J + J.T)


def test_shared_sparse_runs():
    rng = np.random.RandomState(4)
    Ja, Jb, Jc = _sym(rng, 12), _sym(rng, 12), _sym(rng, 10)
    assert not torch.equal(Ja, Jb)
    sa, sb, sc = Ja.to_sparse(), Jb.to_sparse(), Jc.to_sparse()
    runs = B.shared_sparse_runs
    # identity
    assert runs([_Stub(sa)] * 4) == [(0, 4)]
    # the same storage: coalesced tensors that share indices and values
    sa = sa.coalesce()
    twin = torch.sparse_coo_tensor(sa.indices(), sa.values(), sa.shape).coalesce()
    assert runs([_Stub(sa), _Stub(twin)]) == [(0, 2)]
    # equal content in other tensors, uncoalesced and in another entry order included
    idx, val = sa.indices(), sa.values()
    perm = torch.from_numpy(rng.permutation(idx.shape[1]))
    shuffled = torch.sparse_coo_tensor(idx[:, perm], val[perm], sa.shape)
    assert not shuffled.is_coalesced()
    assert runs([_Stub(sa), _Stub(Ja.clone().to_sparse()), _Stub(shuffled)]) == [(0, 3)]
    # one differing value is another J
    other = Ja.clone()
    i, j = [int(x) for x in torch.nonzero(Ja)[0]]
    other[i, j] = other[j, i] = 3.0
    assert runs([_Stub(sa), _Stub(other.to_sparse())]) == []
    # a differing J in the middle splits the runs
    assert runs([_Stub(sa), _Stub(sa), _Stub(sb), _Stub(sa), _Stub(Ja.to_sparse())]) == [(0, 2), (3, 5)]
    # mixed sizes
    assert runs([_Stub(sc), _Stub(sa), _Stub(sa), _Stub(sc), _Stub(sc)]) == [(1, 3), (3, 5)]
    # a dense model ends a run (and never starts one here)
    assert runs([_Stub(sa), _Stub(sa), _Stub(Ja), _Stub(sa)]) == [(0, 2)]
    assert runs([_Stub(Ja), _Stub(Ja)]) == []
    # a run of one is not shared
    assert runs([_Stub(sa)]) == [] and runs([_Stub(sa), _Stub(sb), _Stub(sa)]) == [] and runs([]) == []
    # the dense grouping keeps its answer for sparse models
    assert B.shared_coupling_runs([_Stub(sa), _Stub(sa)]) == []
    assert B.shared_coupling_runs([_Stub(Ja), _Stub(Ja), _Stub(sa)]) == [(0, 2)]


def test_batch_processor_routes_sparse_runs(monkeypatch):
    """No device: a stand-in engine records the setter and the shard each segment of a sparse chunk goes through."""
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

        def set_csr_batch(self, problems):
            calls.append(("set_csr_batch", [len(p[3]) for p in problems]))
            self.n = max(len(p[3]) for p in problems)

        def set_csr_shared(self, rowptr, colidx, val, H):
            calls.append(("set_csr_shared", len(rowptr) - 1, H.shape, [bool(np.any(h)) for h in H]))
            self.n = H.shape[1]

        def describe(self):
            return "csr n=12 shared-J models=3 nnz=1"

        def init_replicas(self, R, seed=0, s0=None, R_global=None, replica0=0):
            calls.append(("init_replicas", R, R_global, replica0))
            self.R = R

        def energies(self):
            return np.zeros(self.R)

        def sweep(self, n_sweeps=1, sched=None):
            pass

        def stats(self):
            return np.zeros(self.R, np.int64), np.ones(self.R, np.int64)

        def best(self, r):
            return 0.0, np.ones(self.n, np.int8), 0

    def model(J, seed):
        m = sg.IsingModel(sg.IsingModelConfig(n_spins=J.shape[0], use_sparse=True))
        m.couplings = J.to_sparse()
        m.set_external_fields(torch.from_numpy(np.random.RandomState(seed).randint(1, 3, J.shape[0]).astype(np.float32)))
        return m

    monkeypatch.setattr(B, "AnnealEngine", Recorder)
    rng = np.random.RandomState(6)
    Ja, Jb, Jc = _sym(rng, 12), _sym(rng, 9), _sym(rng, 12)
    models = [model(Ja, 1), model(Ja, 2), model(Ja, 3), model(Jb, 4), model(Jc, 5), model(Jc, 6)]
    cfg = sg.GPUAnnealerConfig(n_sweeps=10, random_seed=1)
    out = B.BatchProcessor(cfg, B.BatchConfig(replicas_per_model=2)).process_models_batch(models)
    assert len(out) == 6 and calls == [("set_csr_batch", [12, 12, 12, 9, 12, 12]), ("init_replicas", 12, None, 0)], calls
    calls.clear()
    bp = B.BatchProcessor(cfg, B.BatchConfig(replicas_per_model=2, shared_couplings=True))
    out = bp.process_models_batch(models)
    assert len(out) == 6 and all(r is not None for r in out)
    # every segment is the shard of the chunk that starts at its first replica: stand-ins in front, never behind
    assert calls == [("set_csr_shared", 12, (3, 12), [True] * 3), ("init_replicas", 6, None, 0),
                     ("set_csr_batch", [1, 1, 1, 9]), ("init_replicas", 2, 8, 6),
                     ("set_csr_shared", 12, (6, 12), [False] * 4 + [True] * 2), ("init_replicas", 4, 12, 8)], calls
    assert "shared-J" in bp.last_description
