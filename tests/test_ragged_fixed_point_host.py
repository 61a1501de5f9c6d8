"""Fixed-point cached local fields for ragged CSR batches (options "ragged_field_cache" and "clf_fixed_point" together)
without a GPU: the version, the route answers for hand-filled queries, the condition on the test batches (every model
is both accepted and rejected in; the widths and k the batches are built for) and BatchProcessor's two flags."""
import re

import numpy as np

import ragged_fx_cases as fx
from spin_glass_anneal_rl_amd import _native as N

ON, AUTO = 1, 2  # SGA_FIELD_CACHE_ON, SGA_FIELD_CACHE_AUTO
BOTH = {"ragged_field_cache": 1, "clf_fixed_point": 1}


def ragged_query(**kw):
    """What an engine poses for a three-model batch of real-valued short-row models (acc class f64-exact, no table)."""
    base = dict(kind=N.ROUTE_CSR, n=700, n_models=3, R_local=9, nnz=9000, max_row_len=24, layout_entries=9000, acc=2,
                table_m=0, sstride=704, clf_ok=1, clf_bits=32, field_cache=ON)
    opts = kw.pop("options", None)
    return N.route_query(**{**base, **kw, **({"options": opts} if opts else {})})


def cached(**kw):
    return N.explain_route(ragged_query(**kw)).rsplit(" cached=", 1)[1]


def test_version():
    assert N.lib().sga_version() >= 1300


def test_route_with_both_options():
    for bits in (32, 64):
        out = cached(clf_bits=bits, options=BOTH)
        assert out.startswith("on("), out
        assert out == f"on(waves=4 fields=int{bits} fixed-point models=3)", out
    # a row of more than 256 entries: eight waves
    assert cached(max_row_len=257, options=BOTH) == "on(waves=8 fields=int32 fixed-point models=3)"
    # the streaming part of the line is what it is without the options
    assert (N.explain_route(ragged_query(options=BOTH)).rsplit(" cached=", 1)[0]
            == N.explain_route(ragged_query()).rsplit(" cached=", 1)[0])


def test_route_with_either_option_off_is_todays():
    for bits in (32, 64):
        for opts in (None, {"ragged_field_cache": 1}, {"clf_fixed_point": 1}):
            assert cached(clf_bits=bits, options=opts) == "refused", opts  # (the very query that is served above)
            assert cached(clf_bits=bits, options=opts, field_cache=AUTO) == "unavailable", opts
    # a batch the int16 form takes keeps it with both options (the engine reports clf_bits = 16)
    q = dict(acc=0, table_m=60, clf_bits=16)
    assert cached(**q, options=BOTH) == cached(**q, options={"ragged_field_cache": 1}) == "on(waves=4 models=3)"


def test_refusals_with_both_options():
    assert cached(acc=3, options=BOTH) == "refused"            # f64-canonical: no exact fixed point
    assert cached(max_row_len=2100, options=BOTH) == "refused"  # a row past 2048 entries
    assert cached(clf_ok=0, options=BOTH) == "refused"
    assert cached(clf_ok=0, field_cache=AUTO, options=BOTH) == "unavailable"
    # the largest model past LDS: 160 KiB hold ~40 000 int32 | ~20 000 int64 fields beside the spin bits
    for bits, fits, not_ in ((32, 39000, 40000), (64, 19000, 21000)):
        assert cached(clf_bits=bits, n=fits, sstride=fits + 8, options=BOTH).startswith("on("), (bits, fits)
        assert cached(clf_bits=bits, n=not_, sstride=not_, options=BOTH) == "refused", (bits, not_)


def test_auto_break_even_orders_the_widths():
    def theta(bits, **kw):
        out = N.explain_route(ragged_query(field_cache=AUTO, clf_bits=bits, options=BOTH, **kw))
        m = re.search(r"cached=auto\(start=(\w+) theta=([0-9.]+) models=3\)$", out)
        assert m, out
        assert m.group(1) == "rows"  # CSR: a run starts on the row kernels
        return float(m.group(2))
    t64, t32, t16 = theta(64), theta(32), theta(16, acc=0, table_m=60)
    assert t64 < t32 < t16, (t64, t32, t16)


def test_batches_are_what_the_kernel_tests_need():
    want = {"A": ([3, 37, 100, 257, 700], 9, 32, (65, 256)), "B": ([3, 37, 144, 40], None, 64, (1, 256)),
            "C": ([3, 37, 1500], 9, 32, (513, 1024))}
    for name, (sizes, k, bits, (lo, hi)) in want.items():
        probs = fx.batch(name)
        assert fx.rc.sizes(probs) == sizes
        assert lo <= fx.rc.longest_row(probs) <= hi
        kk = fx.batch_k(probs)
        if k is not None:
            assert kk == k
        assert kk >= 9  # model 1's grid is the finest of A and C
        bound = fx.batch_bound(probs)
        assert (bound < 2.0 ** 31) == (bits == 32) and bound < 2.0 ** 53, (name, bound)
        rates = fx.check_acceptance(name)
        assert len(rates) == len(probs)
    A = fx.batch("A")
    assert [fx.lowest_bit_exponent(p[2]) for p in A] == [3, 9, 0, 6, 6]
    # model 2: integer J (the int16 form refuses it for its h alone); h of models 1 and 2 is no multiple of 1/2
    assert np.array_equal(A[2][2], np.rint(A[2][2]))
    for m in (1, 2):
        assert np.any(2 * A[m][3] != np.rint(2 * A[m][3]))
    # batch B's wide model: one pair of 2^22 beside 2^-10 values
    wide = fx.batch("B")[3]
    assert (np.abs(wide[2]) == 2.0 ** 22).sum() == 2 and fx.lowest_bit_exponent(wide[2]) == 10


class _StandIn:
    """Records what BatchProcessor sets on its engine, then refuses the chunk as an engine would (the stacked path is
    not wanted here: the second engine raises for good)."""
    log = []

    def __init__(self, device_index=0):
        self.calls = []
        _StandIn.log.append(self.calls)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def set_field_cache(self, mode):
        self.calls.append(("field_cache", mode))

    def set_option(self, key, value):
        self.calls.append(("option", key, value))

    def set_csr_batch(self, problems):
        self.calls.append(("set_csr_batch", len(problems)))
        raise _Stop()


class _Stop(Exception):
    pass


def test_batch_processor_sets_both_options(monkeypatch):
    import pytest
    import torch
    from spin_glass_anneal_rl_amd import batch as B
    from spin_glass_anneal_rl_amd.gpu_annealer import GPUAnnealerConfig
    from spin_glass_anneal_rl_amd.ising_model import IsingModel, IsingModelConfig

    monkeypatch.setattr(B, "AnnealEngine", _StandIn)
    models = []
    for i, n in enumerate([12, 20]):
        m = IsingModel(IsingModelConfig(n_spins=n, use_sparse=True))
        rp, ci, v = fx.grid_sparse(n, 0.3, 900 + i, 4)
        J = np.zeros((n, n), np.float32)
        for r in range(n):
            J[r, ci[rp[r]:rp[r + 1]]] = v[rp[r]:rp[r + 1]]
        m.set_couplings_from_matrix(torch.from_numpy(J))
        models.append(m)
    for fixed, ragged, want in ((True, True, ["ragged_field_cache", "clf_fixed_point"]), (False, True, ["ragged_field_cache"]),
                                (True, False, []), (False, False, [])):
        _StandIn.log = []
        cfg = GPUAnnealerConfig(n_sweeps=4, random_seed=1, field_cache="on", fixed_point_fields=fixed)
        bp = B.BatchProcessor(cfg, B.BatchConfig(batch_size=4, replicas_per_model=2, ragged_field_cache=ragged))
        with pytest.raises(_Stop):
            bp.process_models_batch(models)
        calls = _StandIn.log[0]
        opts = [c[1] for c in calls if c[0] == "option"]
        assert opts == want, (fixed, ragged, calls)
        assert all(c[2] == 1 for c in calls if c[0] == "option")
        # [set] options: before the couplings
        assert calls[-1] == ("set_csr_batch", 2)
