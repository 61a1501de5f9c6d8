"""Ragged CSR batches without a GPU: the route answer for hand-filled queries and the pure concatenation helper that
AnnealEngine.set_csr_batch runs before any device call."""
import numpy as np
import pytest
import torch

from spin_glass_anneal_rl_amd import _native as N
from spin_glass_anneal_rl_amd.engine import concat_csr_batch
from spin_glass_anneal_rl_amd.exceptions import AnnealingError


def ring(n):
    rp = np.arange(0, 2 * n + 1, 2, dtype=np.int32)
    ci = np.stack([(np.arange(n) - 1) % n, (np.arange(n) + 1) % n], 1).ravel().astype(np.int32)
    return rp, ci, np.ones(2 * n, np.float32), np.zeros(n, np.float32)


def test_explain_route_names_the_narrow_ragged_form():
    q = N.route_query(kind=N.ROUTE_CSR, n=6000, n_models=64, R_local=512, nnz=64 * 3500 * 8, max_row_len=20,
                      layout_entries=64 * 3500 * 8, acc=0, table_m=20)
    out = N.explain_route(q)
    assert out.startswith("csr form=narrow ragged models=64 spins=int8 waves=1 replicas_per_block=4 updates_per_step=1 "), out
    assert "sstride=6000" in out and out.endswith(" cached=off")
    # the field cache is not built for ragged batches; options that would pick another form are errors
    assert N.explain_route(N.route_query(kind=N.ROUTE_CSR, n=100, n_models=3, nnz=300, max_row_len=3, layout_entries=300,
                                         field_cache=1)).endswith(" cached=refused")
    for extra in ({"tune_waves": 2}, {"options": {"force_csr_bits": 1}}, {"options": {"csr_updates_per_step": 4}}):
        q = N.route_query(**{"kind": N.ROUTE_CSR, "n": 100, "n_models": 3, "nnz": 300, "max_row_len": 3,
                             "layout_entries": 300, **extra})
        assert N.explain_route(q).startswith("csr error=ragged CSR batches"), extra
    # the largest model beyond the narrow int8 slice
    q = N.route_query(kind=N.ROUTE_CSR, n=200000, n_models=2, nnz=800000, max_row_len=4, layout_entries=800000)
    assert N.explain_route(q).startswith("csr error=ragged CSR batch: the largest model")


def test_concat_builds_offsets():
    a, b = ring(5), ring(3)
    b_t = tuple(torch.from_numpy(x) for x in b)  # torch works too
    sizes, rp, ci, v, h = concat_csr_batch([a, b_t])
    assert sizes.tolist() == [5, 3] and sizes.dtype == np.int32
    assert rp.dtype == np.int64 and rp.tolist() == list(range(0, 17, 2))
    assert ci.dtype == np.int32 and ci[:10].tolist() == a[1].tolist() and ci[10:].tolist() == b[1].tolist()  # model-local
    assert v.size == 16 and h.size == 8


def test_concat_rejects_bad_input():
    a = ring(4)
    with pytest.raises(AnnealingError):
        concat_csr_batch([])
    with pytest.raises(AnnealingError, match="model 1"):  # length mismatch of colidx / val
        concat_csr_batch([a, (a[0], a[1], a[2][:-1], a[3])])
    with pytest.raises(AnnealingError, match="model 0"):  # h of the wrong length
        concat_csr_batch([(a[0], a[1], a[2], np.zeros(5, np.float32))])
    with pytest.raises(AnnealingError, match="model 0"):  # no spins: a negative / zero size
        concat_csr_batch([(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32))])
    with pytest.raises(AnnealingError, match="model 1"):  # rowptr not ending at nnz
        concat_csr_batch([a, (a[0] + 1, a[1], a[2], a[3])])
    bad = a[1].copy()
    bad[3] = 4  # a column past its model (n = 4)
    with pytest.raises(AnnealingError, match=r"model 1: column index outside \[0, 4\)"):
        concat_csr_batch([ring(9), (a[0], bad, a[2], a[3])])


def test_library_declares_the_batch_entry_points():
    names = [s[0] for s in N.SYMBOLS]
    assert "sga_set_csr_batch" in names and "sga_get_batch_model" in names
