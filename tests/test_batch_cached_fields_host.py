"""Cached local fields for many-model dense batches (sga_set_dense_batch) without a GPU: the form selection's answer for
hand-filled batch queries, unchanged answers for one model (expected strings recorded from the build before the batch
case existed), the documentation and version of the C ABI, and BatchProcessor handing `field_cache` to its engine."""
import os
import re

import numpy as np
import pytest

from spin_glass_anneal_rl_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF, ON, AUTO = 0, 1, 2  # SGA_FIELD_CACHE_*


def int_query(n, R, storage, bits, scale, cache, n_models=1, table_m=20, **kw):
    """What an engine poses for dense integer couplings the cached-field form takes (clf_ok = 1)."""
    elem = 1 if storage in (N.J_I8, N.J_T2) else 4
    ldj = (n * elem + 127) // 128 * 128 // elem
    fields = dict(kind=N.ROUTE_DENSE, n=n, n_models=n_models, R_local=R, storage=storage, acc=0, table_m=table_m, clf_ok=1,
                  clf_bits=bits, clf_scale=scale, field_cache=cache, sstride=ldj)
    fields.update(kw)
    return N.route_query(**fields)


def cached(q):
    return N.explain_route(q).split(" cached=")[1]


def test_version_and_header_document_batches():
    assert N.lib().sga_version() >= 900
    text = open(os.path.join(ROOT, "include", "sga.h")).read()
    cache_doc = re.search(r"/\* How sga_sweep evaluates a proposal\..*?\*/", text, re.S).group(0)
    assert "sga_set_dense_batch" in cache_doc and "dense batches" in cache_doc and "models=M" in cache_doc
    batch_doc = re.search(r"/\* A batch of n_models independent dense problems.*?\*/", text, re.S).group(0)
    assert "sga_set_field_cache" in batch_doc and "batch-wide" in batch_doc


def test_batch_queries_are_served_and_named():
    on = cached(int_query(1000, 16, N.J_I8, 16, 1, ON, n_models=4))
    assert on.startswith("on(") and "models=4" in on and "fields=int16" in on
    on32 = cached(int_query(2500, 8, N.J_F32, 32, 2, ON, n_models=4))
    assert on32.startswith("on(") and "models=4" in on32 and "fields=int32" in on32
    auto = cached(int_query(1000, 16, N.J_I8, 16, 1, AUTO, n_models=4))
    assert auto.startswith("auto(") and "models=4" in auto
    # AUTO's start rule and break-even are those of a lone model of the same size and storage
    lone = cached(int_query(10000, 32, N.J_I8, 16, 1, AUTO))
    member = cached(int_query(10000, 32, N.J_I8, 16, 1, AUTO, n_models=32))
    pat = r"auto\(start=(\w+) theta=([0-9.]+)"
    assert re.match(pat, lone).groups() == re.match(pat, member).groups() == ("cached", "0.387")
    # beyond LDS: 80 000 int16 fields and their spin bits do not fit 160 KiB
    assert cached(int_query(80000, 4, N.J_I8, 16, 1, ON, n_models=4)) == "refused"
    assert cached(int_query(80000, 4, N.J_I8, 16, 1, AUTO, n_models=4)) == "unavailable"
    assert cached(int_query(1000, 16, N.J_I8, 16, 1, OFF, n_models=4)) == "off"
    # a batch that does not qualify (clf_ok = 0) is refused as before
    assert cached(int_query(1000, 16, N.J_I8, 16, 1, ON, n_models=4, clf_ok=0)) == "refused"
    # everything in front of "cached=" is the row kernels' answer, the same with the cache on or off
    a = N.explain_route(int_query(1000, 16, N.J_I8, 16, 1, ON, n_models=4)).split(" cached=")[0]
    b = N.explain_route(int_query(1000, 16, N.J_I8, 16, 1, OFF, n_models=4)).split(" cached=")[0]
    assert a == b


def test_fixed_point_batches_stay_refused():
    # the query of tests/test_dense_fixed_point_host.py::test_refusals: a real-valued batch under option "clf_fixed_point"
    elem, n = 4, 10000
    ldj = (n * elem + 127) // 128 * 128 // elem
    q = N.route_query(kind=N.ROUTE_DENSE, n=n, R_local=1024, storage=N.J_F32, acc=1, table_m=0, clf_ok=0, clf_bits=0,
                      field_cache=ON, sstride=ldj, n_models=4, options={"clf_fixed_point": 1})
    assert cached(q) == "refused"
    q.field_cache = AUTO
    assert cached(q) == "unavailable"


# (n, R, storage, field bits, scale, field cache) -> the answer of the build before batches were served
ONE_MODEL = {
    (1000, 16, N.J_I8, 16, 1, ON): "dense storage=i8 acc=i32 waves=1 chunks_per_wave=1 ld=1024 look_ahead=4 "
                                   "kernel=sweep_dense_kernel cached=on(waves=1 fields=int16)",
    (1000, 16, N.J_I8, 16, 1, AUTO): "dense storage=i8 acc=i32 waves=1 chunks_per_wave=1 ld=1024 look_ahead=4 "
                                     "kernel=sweep_dense_kernel cached=auto(start=rows theta=0.201)",
    (1000, 16, N.J_I8, 16, 1, OFF): "dense storage=i8 acc=i32 waves=1 chunks_per_wave=1 ld=1024 look_ahead=4 "
                                    "kernel=sweep_dense_kernel cached=off",
    (10000, 1024, N.J_I8, 16, 1, ON): "dense storage=i8 acc=i32 waves=2 chunks_per_wave=5 ld=10240 look_ahead=2 "
                                      "kernel=sweep_dense_kernel cached=on(waves=4 fields=int16)",
    (10000, 1024, N.J_I8, 16, 1, AUTO): "dense storage=i8 acc=i32 waves=2 chunks_per_wave=5 ld=10240 look_ahead=2 "
                                        "kernel=sweep_dense_kernel cached=auto(start=cached theta=0.387)",
    (10000, 1024, N.J_T2, 16, 1, AUTO): "dense storage=t2 acc=i32 waves=1 chunks_per_wave=2 ld=16384 look_ahead=4 "
                                        "kernel=sweep_dense_t2_kernel cached=auto(start=rows theta=0.253)",
    (2500, 8, N.J_F32, 32, 2, ON): "dense storage=f32 acc=f32 waves=2 chunks_per_wave=5 ld=2560 look_ahead=2 "
                                   "kernel=sweep_dense_kernel cached=on(waves=4 fields=int32)",
    (2500, 8, N.J_F32, 32, 2, AUTO): "dense storage=f32 acc=f32 waves=2 chunks_per_wave=5 ld=2560 look_ahead=2 "
                                     "kernel=sweep_dense_kernel cached=auto(start=cached theta=0.400)",
    (80000, 4, N.J_I8, 16, 1, ON): "dense storage=i8 acc=i32 waves=16 chunks_per_wave=5 ld=81920 look_ahead=2 "
                                   "kernel=sweep_dense_kernel cached=refused",
    (80000, 4, N.J_I8, 16, 1, AUTO): "dense storage=i8 acc=i32 waves=16 chunks_per_wave=5 ld=81920 look_ahead=2 "
                                     "kernel=sweep_dense_kernel cached=unavailable",
}


@pytest.mark.parametrize("key", sorted(ONE_MODEL))
def test_one_model_answers_are_byte_identical(key):
    assert N.explain_route(int_query(*key)) == ONE_MODEL[key]


def test_batch_processor_hands_field_cache_to_its_engine(monkeypatch):
    """No device: a stand-in engine records the calls BatchProcessor makes, in order."""
    import torch
    import spin_glass_anneal_rl_amd as sg
    from spin_glass_anneal_rl_amd import batch as B

    calls = []

    class Recorder:
        def __init__(self, device=0):
            self.R = 0

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def set_field_cache(self, mode="on"):
            calls.append(("set_field_cache", mode))

        def set_dense_batch(self, J, h, storage="auto"):
            calls.append(("set_dense_batch", J.shape))
            self.n = J.shape[-1]

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
    rng = np.random.RandomState(0)
    models = []
    for m in range(3):
        J = np.triu(rng.randint(0, 2, (12, 12)) * 2 - 1, 1).astype(np.float32)
        model = sg.IsingModel(sg.IsingModelConfig(n_spins=12, use_sparse=False))
        model.set_couplings_from_matrix(torch.from_numpy(J + J.T))
        models.append(model)
    for mode in ("on", "off", "auto"):
        calls.clear()
        cfg = sg.GPUAnnealerConfig(n_sweeps=20, random_seed=1, field_cache=mode)
        out = B.BatchProcessor(cfg, B.BatchConfig(replicas_per_model=2)).process_models_batch(models)
        assert len(out) == 3
        assert calls[0] == ("set_field_cache", mode) and calls[1][0] == "set_dense_batch", calls
