"""AnnealEngine: thin object wrapper over the C ABI handle (include/sga.h).

All arithmetic happens in the HIP kernels behind the handle; this class only marshals
buffers (numpy arrays, or torch tensors whose `data_ptr()` is handed over) and turns status
codes into exceptions.  PyTorch is used for device memory only.
"""
import ctypes as C
import threading
from typing import Optional

import numpy as np

from . import _native as N
from .exceptions import AnnealingError

try:  # torch is plumbing here: device buffers and streams
    import torch
except Exception:  # pragma: no cover
    torch = None


def _is_tensor(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


def _producer_done(t):
    """The engine reads device buffers on its own stream: whatever torch still has queued on its
    current stream to produce `t` must have finished first (free when use_stream() shares it)."""
    if t.is_cuda:
        torch.cuda.current_stream(t.device).synchronize()


def _buf(x, np_dtype, torch_dtype_name, ordered=False):
    """Return (pointer, keepalive) for a numpy array / torch tensor / None.  ordered: the consumer runs
    on the stream that produces the tensor (no wait for the producer)."""
    if x is None:
        return None, None
    if _is_tensor(x):
        want = getattr(torch, torch_dtype_name)
        t = x.detach()
        if t.dtype != want or not t.is_contiguous():
            t = t.to(want).contiguous()
        if not ordered:
            _producer_done(t)
        return C.c_void_p(t.data_ptr()), t
    a = np.ascontiguousarray(x, dtype=np_dtype)
    return a.ctypes.data_as(C.c_void_p), a


def probe_read_bandwidth(device_index: int = 0, nbytes: int = 1 << 32, reps: int = 4) -> float:
    """GB/s of a plain streaming read of a fresh device buffer (sga_probe_read_bandwidth)."""
    out = C.c_double(0.0)
    N.check(N.lib().sga_probe_read_bandwidth(int(device_index), int(nbytes), int(reps), C.byref(out)),
            "sga_probe_read_bandwidth")
    return float(out.value)


def _host_array(x, dtype, what):
    if _is_tensor(x):
        x = x.detach().cpu().numpy()
    a = np.asarray(x)
    if a.ndim != 1:
        raise AnnealingError(f"{what} must be one-dimensional")
    return np.ascontiguousarray(a, dtype=dtype)


def resample_log_q(shift, weight_sum, members: int) -> np.ndarray:
    """ln Q_p = shift[p] + ln(weight_sum[p] / (members * 2^40)) of sga_resample's two exact outputs, float64."""
    w = np.asarray(weight_sum, np.uint64).astype(np.float64)
    return np.asarray(shift, np.float64) + np.log(w / (float(members) * 2.0 ** 40))


def transverse_k_perp(k_perp, n_sweeps: int, n_groups: int) -> np.ndarray:
    """k_perp as sga_sweep_transverse takes it, float32 [n_sweeps, n_groups], from a scalar, [n_sweeps] (one value per
    sweep, shared by the groups) or [n_sweeps, n_groups].  Shapes only: the values are the engine's to judge."""
    n_sweeps, G = max(int(n_sweeps), 0), int(n_groups)
    k = np.asarray(k_perp, dtype=np.float32)
    if k.ndim == 0:
        k = np.full((n_sweeps, G), k, np.float32)
    elif k.shape == (n_sweeps,):
        k = np.repeat(k[:, None], G, axis=1)
    elif k.shape != (n_sweeps, G):
        raise AnnealingError("k_perp must be a scalar, [n_sweeps] or [n_sweeps, R / n_slices]")
    return np.ascontiguousarray(k, dtype=np.float32)


def worldline_p_bond(p_bond, n_sweeps: int, n_groups: int) -> np.ndarray:
    """p_bond as sga_worldline_clusters takes it, float64 [n_sweeps, n_groups], from a scalar, [n_sweeps] (one value per
    sweep, shared by the groups) or [n_sweeps, n_groups].  Shapes only: the values are the engine's to judge."""
    n_sweeps, G = max(int(n_sweeps), 0), int(n_groups)
    b = np.asarray(p_bond, dtype=np.float64)
    if b.ndim == 0:
        b = np.full((n_sweeps, G), b, np.float64)
    elif b.shape == (n_sweeps,):
        b = np.repeat(b[:, None], G, axis=1)
    elif b.shape != (n_sweeps, G):
        raise AnnealingError("p_bond must be a scalar, [n_sweeps] or [n_sweeps, R / n_slices]")
    return np.ascontiguousarray(b, dtype=np.float64)


def concat_csr_batch(problems):
    """[(rowptr, colidx, val, h), ...] (numpy or torch, model-local columns) -> the one concatenated CSR of
    sga_set_csr_batch: (n_spins int32 [M], rowptr int64 [sum n + 1], colidx int32, val float32, h float32).
    Every argument is checked here, before any device call."""
    if isinstance(problems, tuple) or not hasattr(problems, "__len__") or len(problems) == 0:
        raise AnnealingError("problems must be a non-empty list of (rowptr, colidx, val, h)")
    sizes, rps, cis, vals, hs = [], [], [], [], []
    base = 0
    for m, p in enumerate(problems):
        if len(p) != 4:
            raise AnnealingError(f"model {m}: expected (rowptr, colidx, val, h)")
        rp = _host_array(p[0], np.int64, f"model {m}: rowptr")
        ci = _host_array(p[1], np.int64, f"model {m}: colidx")
        v = _host_array(p[2], np.float32, f"model {m}: val")
        h = _host_array(p[3], np.float32, f"model {m}: h")
        n = rp.size - 1
        if n <= 0:
            raise AnnealingError(f"model {m}: rowptr must have n + 1 >= 2 entries")
        if rp[0] != 0 or np.any(np.diff(rp) < 0) or rp[-1] != ci.size:
            raise AnnealingError(f"model {m}: rowptr must start at 0, not decrease and end at len(colidx)")
        if v.size != ci.size:
            raise AnnealingError(f"model {m}: colidx and val differ in length ({ci.size} vs {v.size})")
        if h.size != n:
            raise AnnealingError(f"model {m}: h has {h.size} entries, the model {n} spins")
        if ci.size and (ci.min() < 0 or ci.max() >= n):
            raise AnnealingError(f"model {m}: column index outside [0, {n})")
        sizes.append(n)
        rps.append(rp[:-1] + base if m + 1 < len(problems) else rp + base)
        cis.append(ci.astype(np.int32))
        vals.append(v)
        hs.append(h)
        base += int(rp[-1])
    return (np.asarray(sizes, np.int32), np.concatenate(rps).astype(np.int64), np.concatenate(cis),
            np.concatenate(vals), np.concatenate(hs))


class _SerialisedLib:
    """Calls on one handle must not overlap (include/sga.h); ctypes releases the GIL during a
    call, so the reference's habit of driving sweeps from a thread pool
    (parallel_tempering.py:199, multi_gpu.py:148) is made safe by one lock per engine."""

    def __init__(self, lib):
        self._lib = lib
        self._lock = threading.RLock()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            with self._lock:
                return fn(*args)

        return call


class AnnealEngine:
    """One engine per GPU: packed couplings + R replicas resident in HBM."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        self._lib = _SerialisedLib(N.lib())
        N.check(self._lib.sga_create(int(device), C.byref(self._h)), "sga_create")
        self.device = int(device)
        self.stream_handle = 0
        self.n = 0
        self.R = 0
        self.R_global = 0
        self.replica0 = 0
        self.n_ladders = 0
        self.n_models = 1
        self._sizes = None  # ragged CSR batches: spins of every model

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.sga_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def use_stream(self, stream_handle: Optional[int]):
        N.check(self._lib.sga_set_stream(self._h, C.c_void_p(stream_handle or 0)), "sga_set_stream")
        self.stream_handle = int(stream_handle or 0)

    def shares_torch_stream(self) -> bool:
        """True when the engine launches on torch's current stream of its device: torch work (an RCCL
        collective) and engine kernels are then ordered by the stream, no host synchronisation needed."""
        return bool(self.stream_handle) and torch is not None and torch.cuda.is_available() and \
            self.stream_handle == torch.cuda.current_stream(self.device).cuda_stream

    def problem_checksum(self) -> int:
        out = C.c_uint64(0)
        N.check(self._lib.sga_problem_checksum(self._h, C.byref(out)), "sga_problem_checksum")
        return int(out.value)

    def geometry(self):
        """(waves per replica, chunks per wave) of the dense sweep kernels."""
        w, c = C.c_int(0), C.c_int(0)
        N.check(self._lib.sga_get_geometry(self._h, C.byref(w), C.byref(c)), "sga_get_geometry")
        return int(w.value), int(c.value)

    def set_tuning(self, waves_per_replica: int = 0, sweeps_per_launch: int = 0):
        N.check(self._lib.sga_set_tuning(self._h, int(waves_per_replica), int(sweeps_per_launch)),
                "sga_set_tuning")

    def set_option(self, key: str, value: int):
        """A form-selection option of this engine by name (sga_set_option; keys in include/sga.h).  No option
        changes a result: every form walks the same chain."""
        N.check(self._lib.sga_set_option(self._h, key.encode(), int(value)), "sga_set_option")

    def set_options(self, options=None, **kw):
        """Several options at once: a dict and / or keywords."""
        for k, v in {**(options or {}), **kw}.items():
            self.set_option(k, v)

    def get_option(self, key: str) -> int:
        out = C.c_int64(0)
        N.check(self._lib.sga_get_option(self._h, key.encode(), C.byref(out)), "sga_get_option")
        return int(out.value)

    def set_csr_storage(self, storage: str = "auto"):
        """Entry storage of the long-row CSR sweep forms: "auto" (one dword per entry where the problem
        allows: integer couplings, |J| <= 127, n < 2^24), "f32" (column + fp32 value), "packed" (required)."""
        code = {"auto": 0, "f32": 1, "packed": 2}[storage]
        N.check(self._lib.sga_set_csr_storage(self._h, code), "sga_set_csr_storage")

    def set_field_cache(self, mode="on"):
        """How sweeps evaluate a proposal (sga_set_field_cache): "off" = one coupling-row read per
        proposal (the reference's get_local_field), "on" / "auto" = resident local fields, a row read
        only on accept (the reference's incremental mode); identical chains."""
        code = {"off": 0, False: 0, "on": 1, True: 1, "auto": 2}[mode]
        N.check(self._lib.sga_set_field_cache(self._h, code), "sga_set_field_cache")

    def set_sequential_windows(self, W: int = 1024):
        """Sequential windows (sga_set_sequential_windows): SITE_SEQUENTIAL sweeps of many replicas read each coupling
        row once per sweep -- W = 256 | 512 | 1024 consecutive sites per window, 0 = off (default).  Acts with
        set_field_cache("off") on one dense symmetric matrix whose row sums are exact (integer J and h, or option
        "row_shared_grid" = 1 and J on a grid 2^-k); every other call runs the kernel it had.  Identical chains."""
        N.check(self._lib.sga_set_sequential_windows(self._h, int(W)), "sga_set_sequential_windows")

    def sequential_windows(self) -> int:
        w = C.c_int(0)
        N.check(self._lib.sga_get_sequential_windows(self._h, C.byref(w)), "sga_get_sequential_windows")
        return int(w.value)

    def set_replica_groups(self, g: int = 0):
        """Replica groups (sga_set_replica_groups): the row-shared sweep over the tile plan runs contiguous groups of
        replicas as pipelines of their own, a stream each, joined before the sweep returns -- 0 = the rule's count
        (default), 1 | 2 | 4 = that many where the form admits groups.  Identical chains."""
        N.check(self._lib.sga_set_replica_groups(self._h, int(g)), "sga_set_replica_groups")

    def replica_groups(self) -> int:
        g = C.c_int(0)
        N.check(self._lib.sga_get_replica_groups(self._h, C.byref(g)), "sga_get_replica_groups")
        return int(g.value)

    def autotune(self) -> float:
        """Time every feasible waves-per-replica on the current replicas and keep the fastest
        (dense problems; results are unaffected).  Returns the best kernel ms per sweep."""
        ms = C.c_double(0.0)
        N.check(self._lib.sga_autotune(self._h, C.byref(ms)), "sga_autotune")
        return float(ms.value)

    def autotune_table(self, forms: bool = False) -> dict:
        """{candidate: kernel ms per sweep} of the last autotune() (dense: "<waves>x<chunks per wave>").  `forms=True`
        adds the other sweep forms it timed beside the geometries ("row-shared:W<W>", option "row_shared")."""
        buf = C.create_string_buffer(4096)
        N.check(self._lib.sga_get_autotune_table(self._h, buf, 4096), "sga_get_autotune_table")
        out = {}
        for item in buf.value.decode().split(";"):
            if "=" in item:
                k, v = item.rsplit("=", 1)
                if forms or not k.startswith("row-shared:"):
                    out[k] = float(v)
        return out

    def maybe_autotune(self, n_sweeps: int, setting: Optional[bool] = None) -> bool:
        """Host-loop helper: autotune when asked to (`setting=True`), never when `False`, and by
        default (`None`) only when the run is long enough to pay for the ~30 trial sweeps."""
        if setting is False or self.R <= 0:
            return False
        if setting is None and float(self.n) ** 2 * self.R * n_sweeps < 2e13:
            return False
        if setting is None and "sweep=cached-local-fields" in self.describe():
            return False  # the measured geometry belongs to the row-per-proposal kernels
        self.autotune()
        return True

    # ------------------------------------------------------------------ problem
    def set_dense(self, J, h, storage: str = "auto"):
        sel = {"auto": N.J_AUTO, "f32": N.J_F32, "i8": N.J_I8, "t2": N.J_T2}[storage]
        if _is_tensor(J):
            if J.dim() != 2 or J.shape[0] != J.shape[1]:
                raise AnnealingError("couplings must be a square matrix")
            Jt = J.detach()
            if Jt.dtype != torch.float32:
                Jt = Jt.float()
            if Jt.stride(1) != 1:
                Jt = Jt.contiguous()
            _producer_done(Jt)
            n, ld, jp, keep = Jt.shape[0], Jt.stride(0), C.c_void_p(Jt.data_ptr()), Jt
        else:
            Ja = np.ascontiguousarray(J, dtype=np.float32)
            if Ja.ndim != 2 or Ja.shape[0] != Ja.shape[1]:
                raise AnnealingError("couplings must be a square matrix")
            n, ld, jp, keep = Ja.shape[0], Ja.shape[1], Ja.ctypes.data_as(C.c_void_p), Ja
        hp, hk = _buf(h, np.float32, "float32")
        if (hk.numel() if _is_tensor(hk) else hk.size) != n:
            raise AnnealingError("external fields must have n entries")
        N.check(self._lib.sga_set_dense(self._h, jp, int(ld), hp, int(n), sel), "sga_set_dense")
        del keep
        self._sizes = None
        self.n, self.R, self.n_models = n, 0, 1

    def set_dense_batch(self, J, h, storage: str = "auto"):
        """Many independent models of one size: J [M, n, n], h [M, n] (numpy or torch)."""
        sel = {"auto": N.J_AUTO, "f32": N.J_F32, "i8": N.J_I8, "t2": N.J_T2}[storage]
        if _is_tensor(J):
            Jt = J.detach().float().contiguous()
            _producer_done(Jt)
            M, n = Jt.shape[0], Jt.shape[1]
            jp, keep = C.c_void_p(Jt.data_ptr()), Jt
        else:
            Ja = np.ascontiguousarray(J, dtype=np.float32)
            M, n = Ja.shape[0], Ja.shape[1]
            jp, keep = Ja.ctypes.data_as(C.c_void_p), Ja
        if keep.ndim != 3 or keep.shape[2] != n:
            raise AnnealingError("batched couplings must be [M, n, n]")
        hp, hk = _buf(h, np.float32, "float32")
        if (hk.numel() if _is_tensor(hk) else hk.size) != M * n:
            raise AnnealingError("batched fields must be [M, n]")
        N.check(self._lib.sga_set_dense_batch(self._h, jp, int(n), hp, int(n), int(M), sel),
                "sga_set_dense_batch")
        del keep
        self._sizes = None
        self.n, self.R, self.n_models = n, 0, M

    def set_dense_shared(self, J, H, storage: str = "auto"):
        """One coupling matrix under many field vectors (sga_set_dense_shared): J [n, n], H [M, n] (numpy or torch, host
        or device).  The engine behaves as after set_dense_batch on J tiled M times -- replicas split evenly over the M
        models, one ladder per model -- but holds J once, serves storage="t2" and opens the row-shared windows and the
        matrix-core energy pass to the batch."""
        sel = {"auto": N.J_AUTO, "f32": N.J_F32, "i8": N.J_I8, "t2": N.J_T2}[storage]
        if _is_tensor(J):
            if J.dim() != 2 or J.shape[0] != J.shape[1]:
                raise AnnealingError("shared couplings must be a square matrix [n, n]")
            Jt = J.detach()
            if Jt.dtype != torch.float32:
                Jt = Jt.float()
            if Jt.stride(1) != 1:
                Jt = Jt.contiguous()
            _producer_done(Jt)
            n, ld, jp, keep = Jt.shape[0], Jt.stride(0), C.c_void_p(Jt.data_ptr()), Jt
        else:
            Ja = np.ascontiguousarray(J, dtype=np.float32)
            if Ja.ndim != 2 or Ja.shape[0] != Ja.shape[1]:
                raise AnnealingError("shared couplings must be a square matrix [n, n]")
            n, ld, jp, keep = Ja.shape[0], Ja.shape[1], Ja.ctypes.data_as(C.c_void_p), Ja
        if not _is_tensor(H):
            H = np.asarray(H, dtype=np.float32)
        if H.ndim != 2 or H.shape[1] != n or H.shape[0] < 1:
            raise AnnealingError("shared-coupling fields must be [M, n]")
        M = int(H.shape[0])
        hp, hk = _buf(H, np.float32, "float32")
        N.check(self._lib.sga_set_dense_shared(self._h, jp, int(ld), hp, int(n), M, sel), "sga_set_dense_shared")
        del keep, hk
        self._sizes = None
        self.n, self.R, self.n_models = n, 0, M

    def set_csr(self, rowptr, colidx, val, h):
        """CSR couplings (both triangles).  int64 `rowptr` (numpy / torch) is passed through as
        64-bit extents -- required once nnz >= 2^31 -- anything else is taken as int32."""
        wide = getattr(rowptr, "dtype", None) in ((np.dtype(np.int64),) + ((torch.int64,) if torch is not None else ()))
        rp, k1 = _buf(rowptr, np.int64, "int64") if wide else _buf(rowptr, np.int32, "int32")
        ci, k2 = _buf(colidx, np.int32, "int32")
        vp, k3 = _buf(val, np.float32, "float32")
        hp, k4 = _buf(h, np.float32, "float32")
        n = (k1.numel() if _is_tensor(k1) else k1.size) - 1
        nnz = k2.numel() if _is_tensor(k2) else k2.size
        if k3 is not None and (k3.numel() if _is_tensor(k3) else k3.size) != nnz:  # (the C call reads nnz values, n fields)
            raise AnnealingError("CSR values must have one entry per column index")
        if k4 is not None and (k4.numel() if _is_tensor(k4) else k4.size) != n:
            raise AnnealingError("external fields must have n entries")
        fn, name = (self._lib.sga_set_csr64, "sga_set_csr64") if wide else (self._lib.sga_set_csr, "sga_set_csr")
        N.check(fn(self._h, rp, ci, vp, hp, int(n), int(nnz)), name)
        self.n, self.R, self.n_models = n, 0, 1
        self._sizes = None

    def set_csr_shared(self, rowptr, colidx, val, H):
        """One set of CSR rows under many field vectors (sga_set_csr_shared): rowptr [n + 1], colidx, val as in set_csr
        (int32 extents), H [M, n] (numpy or torch, host or device).  Replicas are split evenly over the M models, one
        ladder per model; the entries are held once and every one-wave-per-replica CSR form is served.  A refused input
        (bad extents, a column out of range, a non-finite value) leaves the problem the engine held in place."""
        rp, k1 = _buf(rowptr, np.int32, "int32")
        ci, k2 = _buf(colidx, np.int32, "int32")
        vp, k3 = _buf(val, np.float32, "float32")
        n = (k1.numel() if _is_tensor(k1) else k1.size) - 1
        nnz = k2.numel() if _is_tensor(k2) else k2.size
        if k3 is not None and (k3.numel() if _is_tensor(k3) else k3.size) != nnz:
            raise AnnealingError("CSR values must have one entry per column index")
        if not _is_tensor(H):
            H = np.asarray(H, dtype=np.float32)
        if H.ndim != 2 or H.shape[1] != n or H.shape[0] < 1:
            raise AnnealingError("shared-coupling fields must be [M, n]")
        M = int(H.shape[0])
        hp, k4 = _buf(H, np.float32, "float32")
        N.check(self._lib.sga_set_csr_shared(self._h, rp, ci, vp, hp, int(n), int(nnz), M), "sga_set_csr_shared")
        del k1, k2, k3, k4
        self.n, self.R, self.n_models = n, 0, M
        self._sizes = None

    def set_csr_batch(self, problems):
        """Many independent sparse models of any sizes in one engine (sga_set_csr_batch): `problems` is a list of
        (rowptr, colidx, val, h) with model-local columns.  Replicas are split evenly over the models (R a multiple of
        the number of models); spins(r) and best(r) return the n of replica r's model."""
        sizes, rp, ci, v, h = concat_csr_batch(problems)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        N.check(self._lib.sga_set_csr_batch(self._h, int(sizes.size), ptr(sizes), ptr(rp), ptr(ci), ptr(v), ptr(h),
                                            int(ci.size)), "sga_set_csr_batch")
        self.n, self.R, self.n_models = int(sizes.max()), 0, int(sizes.size)
        self._sizes = sizes

    def model_sizes(self) -> np.ndarray:
        """Spins of every model (one entry per model; dense batches and single problems: n each)."""
        sizes = getattr(self, "_sizes", None)
        return sizes.copy() if sizes is not None else np.full(self.n_models, self.n, np.int32)

    def _replica_n(self, r: int) -> int:
        sizes = getattr(self, "_sizes", None)
        if sizes is None:
            return self.n
        return int(sizes[(self.replica0 + int(r)) // (self.R_global // sizes.size)])

    def set_tsp(self, dist, city_visit: float, position_fill: float, h):
        """TSP-structured couplings, never stored (see sga_set_tsp): dist [n, n] float32 (numpy or
        torch), the two penalty weights as the encoder scaled them, and the fields h [n * n]
        (`encoders.tsp_structure` returns all four)."""
        if _is_tensor(dist):
            dt = dist.detach().float()
            if dt.dim() != 2 or dt.shape[0] != dt.shape[1]:
                raise AnnealingError("the distance matrix must be square")
            if dt.stride(1) != 1:
                dt = dt.contiguous()
            _producer_done(dt)
            n, ld, dp, keep = dt.shape[0], dt.stride(0), C.c_void_p(dt.data_ptr()), dt
        else:
            da = np.ascontiguousarray(dist, dtype=np.float32)
            if da.ndim != 2 or da.shape[0] != da.shape[1]:
                raise AnnealingError("the distance matrix must be square")
            n, ld, dp, keep = da.shape[0], da.shape[1], da.ctypes.data_as(C.c_void_p), da
        hp, hk = _buf(h, np.float32, "float32")
        if (hk.numel() if _is_tensor(hk) else hk.size) != n * n:
            raise AnnealingError("the fields must have n_cities^2 entries")
        N.check(self._lib.sga_set_tsp(self._h, dp, int(ld), int(n), float(city_visit), float(position_fill),
                                      hp), "sga_set_tsp")
        del keep
        self._sizes = None
        self.n, self.R, self.n_models = n * n, 0, 1

    def set_groups(self, n: int, groups, coeff, h, rest=None):
        """Couplings that are a sum of complete graphs on groups of sites, never stored (see sga_set_groups):
        J_ij = sum of coeff[g] over the groups that hold both i and j.  `groups` is a list of index arrays or a
        tuple (member_ptr int64 [G + 1], members int32); `coeff` [G] and `h` [n] float32; numpy or torch device
        tensors (`encoders.assignment_groups` / `scheduling_groups` / `IsingBuilder.group_structure` return them).
        `rest`: a stored sparse remainder R added to those couplings (see sga_set_groups_csr) -- (rowptr int32 [n + 1],
        colidx int32, val float32) or a scipy sparse matrix; symmetric, zero diagonal, rows strictly sorted and at most
        256 entries long (`IsingBuilder.group_rest_structure` / `encoders.scheduling_groups_rest` return it)."""
        if isinstance(groups, tuple) and len(groups) == 2:  # (a LIST of two index arrays is two groups)
            member_ptr, members = groups
        else:
            rows = [np.asarray(g, np.int32).ravel() for g in groups]
            member_ptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
            members = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
        if rest is not None and hasattr(rest, "tocsr"):
            m = rest.tocsr()
            m.sum_duplicates()
            m.sort_indices()
            rest = (np.asarray(m.indptr, np.int32), np.asarray(m.indices, np.int32), np.asarray(m.data, np.float32))
        mp, k1 = _buf(member_ptr, np.int64, "int64")
        mm, k2 = _buf(members, np.int32, "int32")
        cp, k3 = _buf(coeff, np.float32, "float32")
        hp, k4 = _buf(h, np.float32, "float32")
        size = lambda k: 0 if k is None else (k.numel() if _is_tensor(k) else k.size)  # noqa: E731
        G = size(k1) - 1
        if size(k3) != G:
            raise AnnealingError("one coefficient per group")
        if size(k4) != int(n):
            raise AnnealingError("external fields must have n entries")
        if rest is None:
            N.check(self._lib.sga_set_groups(self._h, int(n), int(G), mp, mm, cp, hp), "sga_set_groups")
        else:
            rowptr, colidx, val = rest
            rp, k5 = _buf(rowptr, np.int32, "int32")
            ci, k6 = _buf(colidx, np.int32, "int32")
            vp, k7 = _buf(val, np.float32, "float32")
            if size(k5) != int(n) + 1:
                raise AnnealingError("the remainder's rowptr must have n + 1 entries")
            if size(k6) != size(k7):
                raise AnnealingError("the remainder needs one value per column index")
            N.check(self._lib.sga_set_groups_csr(self._h, int(n), int(G), mp, mm, cp, rp, ci, vp, int(size(k7)), hp),
                    "sga_set_groups_csr")
            del k5, k6, k7
        del k1, k2, k3, k4
        self._sizes = None
        self.n, self.R, self.n_models = int(n), 0, 1

    # ------------------------------------------------------------------ replicas
    def init_replicas(self, R: int, seed: int = 0, s0=None, R_global: Optional[int] = None,
                      replica0: int = 0):
        Rg = R if R_global is None else int(R_global)
        sp, keep = _buf(s0, np.int8, "int8")
        if keep is not None:
            cnt = keep.numel() if _is_tensor(keep) else keep.size
            if cnt != R * self.n:
                raise AnnealingError("s0 must be [R, n] int8")
        self.R = 0  # a failed call leaves the engine without replicas (include/sga.h)
        N.check(self._lib.sga_init_replicas(self._h, int(R), Rg, int(replica0),
                                            int(seed) & 0xFFFFFFFFFFFFFFFF, sp),
                "sga_init_replicas")
        self.R, self.R_global, self.replica0, self.n_ladders = int(R), Rg, int(replica0), 0

    def set_temperatures(self, T):
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(T, np.float64), (self.R,)))
        N.check(self._lib.sga_set_temperatures(self._h, t.ctypes.data_as(C.c_void_p)),
                "sga_set_temperatures")

    def set_ladder(self, slot_temps, n_ladders: int = 1):
        t = np.ascontiguousarray(slot_temps, dtype=np.float64)
        if t.size != self.R_global:
            raise AnnealingError("slot_temps must have R_global entries")
        N.check(self._lib.sga_set_ladder(self._h, t.ctypes.data_as(C.c_void_p), int(n_ladders)),
                "sga_set_ladder")
        self.n_ladders = int(n_ladders)

    # ------------------------------------------------------------------ hot path
    def sweep(self, n_sweeps: int = 1, site_mode: int = N.SITE_RANDOM, arith: int = N.ARITH_F64,
              sched=None, replay_site=None, replay_u=None, energy_trace: bool = False,
              trace: bool = False):
        """n_sweeps Metropolis sweeps of every replica.

        sched: None | [n_sweeps] (shared by all replicas) | [n_sweeps, R] temperatures.
        Returns {"energy_trace": [n_sweeps, R] | None, "accept_trace", "dE_trace"}.
        """
        n_sweeps = int(n_sweeps)
        sp, ss, rs, keep_s = None, 0, 0, None
        if sched is not None:
            keep_s = np.ascontiguousarray(sched, dtype=np.float64)
            if keep_s.ndim == 1 and keep_s.shape[0] == n_sweeps:
                ss, rs = 1, 0
            elif keep_s.shape == (n_sweeps, self.R):
                ss, rs = self.R, 1
            else:
                raise AnnealingError("sched must be [n_sweeps] or [n_sweeps, R]")
            sp = keep_s.ctypes.data_as(C.c_void_p)
        per = n_sweeps * self.n
        rsp, k1 = _buf(replay_site, np.int32, "int32")
        rup, k2 = _buf(replay_u, np.float32, "float32")
        for k in (k1, k2):
            if k is not None and (k.numel() if _is_tensor(k) else k.size) != self.R * per:
                raise AnnealingError("replay arrays must be [R, n_sweeps*n]")
        et = np.zeros((n_sweeps, self.R), np.float64) if energy_trace else None
        at = np.zeros((self.R, per), np.uint8) if trace else None
        dt = np.zeros((self.R, per), np.float64) if trace else None
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        N.check(self._lib.sga_sweep(self._h, n_sweeps, int(site_mode), int(arith), sp, ss, rs, rsp,
                                    rup, ptr(et), ptr(at), ptr(dt)), "sga_sweep")
        return {"energy_trace": et, "accept_trace": at, "dE_trace": dt}

    # ------------------------------------------------------------------ simulated quantum annealing
    def _trotter_groups(self, P: int) -> int:
        """R / P groups of P slices -- for a P the engine will refuse, 1: any well-formed array then does, so that the
        refusal and its reason are the engine's."""
        return self.R // P if P >= 1 and self.R > 0 and self.R % P == 0 else 1

    def sweep_transverse(self, n_sweeps: int, n_slices: int, k_perp, arith: int = N.ARITH_F64):
        """n_sweeps sweeps of the replicas as R / n_slices groups of n_slices Trotter slices (sga_sweep_transverse): per
        sweep the even slices move under h + k (s_up + s_dn), then the odd ones; the tracked energies stay classical.
        k_perp: a scalar, [n_sweeps] or [n_sweeps, R / n_slices] (see quantum.transverse_coupling).  A problem the step
        does not serve raises AnnealingError with the engine's reason."""
        G = self._trotter_groups(int(n_slices))
        k = transverse_k_perp(k_perp, n_sweeps, G)
        N.check(self._lib.sga_sweep_transverse(self._h, int(n_sweeps), int(n_slices), int(arith), k.ctypes.data_as(C.c_void_p)),
                "sga_sweep_transverse")

    def sweep_transverse_dense(self, n_sweeps: int, n_slices: int, k_perp, arith: int = N.ARITH_F64):
        """sweep_transverse on one dense matrix (sga_sweep_transverse_dense): the same step, carried by the cached local
        fields -- a moving slice keeps its fields in LDS and reads a coupling row only on accept; the fields are seeded
        where they are not valid and stay valid for a cached sweep() after it.  k_perp as in sweep_transverse.  Serves
        integer symmetric J with a zero diagonal and h in multiples of 1/2 (set_dense); with option "clf_fixed_point" = 1
        set before set_dense also real-valued symmetric J on a binary grid with a zero diagonal and any h, on exact
        fixed-point fields (int32 | int64).  Any other problem raises AnnealingError with the engine's reason."""
        G = self._trotter_groups(int(n_slices))
        k = transverse_k_perp(k_perp, n_sweeps, G)
        N.check(self._lib.sga_sweep_transverse_dense(self._h, int(n_sweeps), int(n_slices), int(arith), k.ctypes.data_as(C.c_void_p)),
                "sga_sweep_transverse_dense")

    def worldline_clusters(self, n_sweeps: int, n_slices: int, p_bond, round: Optional[int] = None, stats: bool = False):
        """n_sweeps sweeps of world-line cluster updates over the replicas as R / n_slices groups of n_slices Trotter
        slices (sga_worldline_clusters): per site the slices are cut into segments by bonds drawn with p_bond between equal
        neighbouring slices (see quantum.bond_probability), and each segment flips as one under the classical field; the
        tracked energies stay classical.  p_bond: a scalar, [n_sweeps] or [n_sweeps, R / n_slices].  round: the draws'
        coordinate, None = the engine's sweeps_done (counters()[0]); sweep kk draws at round + kk.  stats=True returns
        int64 [R / n_slices, 3]: segments formed, segments flipped, slice spins flipped.  A problem the step does not
        serve raises AnnealingError with the engine's reason."""
        P = int(n_slices)
        G = self._trotter_groups(P)
        b = worldline_p_bond(p_bond, n_sweeps, G)
        rnd = self.counters()[0] if round is None else int(round)
        out = np.zeros((G, 3), np.int64) if stats else None
        N.check(self._lib.sga_worldline_clusters(self._h, int(n_sweeps), P, rnd & 0xFFFFFFFF, b.ctypes.data_as(C.c_void_p),
                                                 out.ctypes.data_as(C.c_void_p) if stats else None), "sga_worldline_clusters")
        return out

    def worldline_clusters_dense(self, n_sweeps: int, n_slices: int, p_bond, round: Optional[int] = None, stats: bool = False):
        """worldline_clusters on one dense matrix (sga_worldline_clusters_dense): the same step, decided on the cached local
        fields of every slice -- a coupling row is read only where a segment flips, and the fields are seeded where they
        are not valid and stay valid: sweep_transverse_dense, this call, sweep_transverse_dense run without seeding in
        between.  Arguments and the returned statistics as in worldline_clusters.  Serves what sweep_transverse_dense
        serves, whatever the update rule; any other problem raises AnnealingError with the engine's reason."""
        P = int(n_slices)
        G = self._trotter_groups(P)
        b = worldline_p_bond(p_bond, n_sweeps, G)
        rnd = self.counters()[0] if round is None else int(round)
        out = np.zeros((G, 3), np.int64) if stats else None
        N.check(self._lib.sga_worldline_clusters_dense(self._h, int(n_sweeps), P, rnd & 0xFFFFFFFF, b.ctypes.data_as(C.c_void_p),
                                                       out.ctypes.data_as(C.c_void_p) if stats else None),
                "sga_worldline_clusters_dense")
        return out

    def time_links(self, n_slices: int, out=None):
        """int64 [R / n_slices]: the broken time links B_g of every group of n_slices Trotter slices (sga_get_time_links):
        the sites at which neighbouring slices of the ring differ, summed over the ring (n_slices = 2: a differing site
        counts 2).  All that quantum.transverse_magnetization and quantum.quantum_energy read of the spins.  Read only;
        any n_slices >= 2 that divides R.  out: an optional contiguous int64 CUDA tensor [R / n_slices] that receives the
        counts on the device, under the conventions of overlaps(out=): with shares_torch_stream() the call is only
        enqueued."""
        P = int(n_slices)
        G = self._trotter_groups(P)
        ptr, res, dev = self._pair_out(out, G, "int64", "out")
        N.check(self._lib.sga_get_time_links(self._h, P, ptr), "sga_get_time_links")
        self._observable_done(dev)
        if dev:
            self._pending = (res,)  # a device result stays alive while the work is queued
        return res

    def exchange_transverse(self, n_slices: int, k_perp, parity: Optional[int] = None, round: Optional[int] = None):
        """One round of replica exchange between neighbouring groups of n_slices Trotter slices along the transverse
        field (sga_exchange_transverse): the pairs (a, a + 1) with a % 2 == parity swap with probability
        min(1, exp[(beta_a - beta_b)(E_a - E_b) + 2 (beta_a k_a - beta_b k_b)(B_a - B_b)]) -- whole groups trade spin
        rows, tracked energies and, where they are valid, cached local fields, which stay valid.  k_perp: a scalar or
        [R / n_slices], the couplings the groups run at.  round: None = counters()[0]; parity: None = round & 1.  No
        counter, temperature or statistic of the engine moves.  Returns (accepted int32 [G], links int64 [G]): 1 for
        both groups of a swapped pair, and B of every group before the exchange."""
        P = int(n_slices)
        G = self._trotter_groups(P)
        k = np.asarray(k_perp, dtype=np.float32)
        if k.ndim == 0:
            k = np.full(G, k, np.float32)
        elif k.shape != (G,):
            raise AnnealingError("k_perp must be a scalar or [R / n_slices]")
        k = np.ascontiguousarray(k, dtype=np.float32)
        rnd = self.counters()[0] if round is None else int(round)
        par = (rnd & 1) if parity is None else int(parity)
        accepted, links = np.zeros(G, np.int32), np.zeros(G, np.int64)
        N.check(self._lib.sga_exchange_transverse(self._h, P, k.ctypes.data_as(C.c_void_p), par, rnd & 0xFFFFFFFF,
                                                  accepted.ctypes.data_as(C.c_void_p), links.ctypes.data_as(C.c_void_p)),
                "sga_exchange_transverse")
        return accepted, links

    # single-site operators (the reference's per-spin API)
    def local_fields(self, r: int, sites) -> np.ndarray:
        idx = np.ascontiguousarray(np.atleast_1d(sites), dtype=np.int32)
        out = np.zeros(idx.size, np.float64)
        N.check(self._lib.sga_local_fields(self._h, int(r), idx.ctypes.data_as(C.c_void_p),
                                           int(idx.size), out.ctypes.data_as(C.c_void_p)),
                "sga_local_fields")
        return out

    def flip(self, r: int, site: int) -> float:
        d = C.c_double(0.0)
        N.check(self._lib.sga_flip(self._h, int(r), int(site), C.byref(d)), "sga_flip")
        return float(d.value)

    def update(self, r: int, site: int, T: float, u: float, arith: int = N.ARITH_F64):
        acc, d = C.c_int(0), C.c_double(0.0)
        N.check(self._lib.sga_update(self._h, int(r), int(site), float(T), float(u), int(arith),
                                     C.byref(acc), C.byref(d)), "sga_update")
        return bool(acc.value), float(d.value)

    def set_update_rule(self, rule: int):
        N.check(self._lib.sga_set_update_rule(self._h, int(rule)), "sga_set_update_rule")

    def set_wolff_replay(self, u):
        """Recorded uniforms for the Wolff rule's candidate bonds, [R, capacity] float32, consumed in
        draw order by the following Wolff sweeps (parity tests); None: back to Philox."""
        if u is None:
            N.check(self._lib.sga_set_wolff_replay(self._h, None, 0), "sga_set_wolff_replay")
            return
        a = np.ascontiguousarray(u, dtype=np.float32).reshape(self.R, -1)
        N.check(self._lib.sga_set_wolff_replay(self._h, a.ctypes.data_as(C.c_void_p), int(a.shape[1])),
                "sga_set_wolff_replay")

    def recompute_energies(self):
        N.check(self._lib.sga_recompute_energies(self._h), "sga_recompute_energies")

    def exchange(self, energies_global=None, start=None, u=None, count: bool = True):
        """One exchange round.  With count=False the call only enqueues the kernel (no host
        synchronisation) and returns None -- use it inside sweep / exchange loops."""
        ep, k1 = _buf(energies_global, np.float64, "float64",
                      ordered=_is_tensor(energies_global) and energies_global.is_cuda and self.shares_torch_stream())
        stp, k2 = _buf(None if start is None else np.atleast_1d(start), np.int32, "int32")
        up, k3 = _buf(u, np.float64, "float64")
        if not count:
            N.check(self._lib.sga_exchange(self._h, ep, stp, up, None), "sga_exchange")
            self._pending = (k1, k2, k3)  # converted device tensors stay alive while the kernel is queued
            return None
        out = C.c_int(0)
        N.check(self._lib.sga_exchange(self._h, ep, stp, up, C.byref(out)), "sga_exchange")
        return int(out.value)

    def exchange_pairs(self, pairs, u=None, energies_global=None) -> int:
        """Exchange attempts over an ordered list of slot pairs [(i, j), ...], each seeing the
        swaps before it (the reference's exchange_method="all_pairs").  Returns the accepted count."""
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        ep, k1 = _buf(energies_global, np.float64, "float64")
        up, k2 = _buf(u, np.float64, "float64")
        if k2 is not None and (k2.numel() if _is_tensor(k2) else k2.size) != len(pr):
            raise AnnealingError("u must have one entry per pair")
        out = C.c_int(0)
        N.check(self._lib.sga_exchange_pairs(self._h, ep, pr.ctypes.data_as(C.c_void_p), up, len(pr),
                                             C.byref(out)), "sga_exchange_pairs")
        return int(out.value)

    # ------------------------------------------------------------------ isoenergetic cluster moves
    # csrc/cluster_moves.hip: between two replicas of one sparse Hamiltonian AT EQUAL TEMPERATURES (the caller's to see
    # to), the connected component of differing sites around one drawn site is flipped in both; E_a + E_b is conserved.
    def _cluster_sizes(self, sizes, count: int):
        """(pointer, result, device?) of a cluster call's sizes: True a fresh int32 numpy array, False / None nothing, an
        int32 CUDA tensor of `count` entries the caller's buffer (the call is then only enqueued)."""
        if sizes is None or sizes is False:
            return None, None, False
        if sizes is True:
            res = np.zeros(count, np.int32)
            return res.ctypes.data_as(C.c_void_p), res, False
        if not _is_tensor(sizes) or not sizes.is_cuda or sizes.dtype != torch.int32 or sizes.numel() != count or \
                not sizes.is_contiguous():
            raise AnnealingError(f"sizes must be True, False or a contiguous int32 CUDA tensor of {count} entries")
        if not self.shares_torch_stream():
            _producer_done(sizes)
        return C.c_void_p(sizes.data_ptr()), sizes, True

    def cluster_move_pairs(self, pairs, round: Optional[int] = None, sizes=True):
        """One isoenergetic cluster move per pair (a, b) of LOCAL replica indices (sga_cluster_move_pairs): every replica
        at most once, a != b; CSR couplings only.  round: the draw's coordinate, None = the engine's exchange-round
        counter (counters()[1]).  Returns the clusters' sizes, int32 [count] (sizes=False: None; a CUDA tensor: filled
        on the device, the call only enqueued)."""
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        rnd = self.counters()[1] if round is None else int(round)
        ptr, res, dev = self._cluster_sizes(sizes, len(pr))
        N.check(self._lib.sga_cluster_move_pairs(self._h, pr.ctypes.data_as(C.c_void_p), len(pr), rnd & 0xFFFFFFFF, ptr),
                "sga_cluster_move_pairs")
        self._observable_done(dev)
        self._pending = (pr, res)  # the pair list and a device result stay alive while the work is queued
        return res

    def cluster_move_ladders(self, slot_lo: int = 0, slot_hi: Optional[int] = None, round: Optional[int] = None, sizes=True):
        """One isoenergetic cluster move per slot slot_lo <= s < slot_hi (None: every slot) and pair of ladders 2c, 2c + 1,
        between the replicas that hold slot s of both now -- read from the slot map on the device, no host round trip
        (sga_cluster_move_ladders; an even n_ladders, every replica local).  Returns the sizes as int32
        [n_ladders / 2, slot_hi - slot_lo] (sizes=False: None; a CUDA tensor of as many entries: filled on the device)."""
        if self.n_ladders <= 0:
            raise AnnealingError("no ladder (call set_ladder)")
        L = self.R_global // self.n_ladders
        lo, hi = int(slot_lo), L if slot_hi is None else int(slot_hi)
        rnd = self.counters()[1] if round is None else int(round)
        count = (self.n_ladders // 2) * max(hi - lo, 0)
        ptr, res, dev = self._cluster_sizes(sizes, count)
        N.check(self._lib.sga_cluster_move_ladders(self._h, lo, hi, rnd & 0xFFFFFFFF, ptr), "sga_cluster_move_ladders")
        self._observable_done(dev)
        if res is not None and not dev:
            res = res.reshape(self.n_ladders // 2, max(hi - lo, 0))
        return res

    # ------------------------------------------------------------------ population annealing
    def resample(self, dbeta, n_populations: int = 1, round: Optional[int] = None, parents=True):
        """The resampling step of population annealing (sga_resample, csrc/resample.hip): the local replicas in
        n_populations contiguous populations, every member copied or culled in proportion to exp(-dbeta E), planned and
        copied on the device, exact in integers.  dbeta: a number or one per population.  round: the draw's coordinate,
        None = the engine's exchange-round counter (counters()[1]).  Returns (parents, log_q): parents int32 [R], the
        local index of every slot's parent (parents=False: None), and log_q float64 [n_populations], the free-energy
        increments ln Q_p of the step.  With an int32 CUDA tensor of R entries for `parents` the call is only enqueued:
        the tensor is filled on the device and log_q comes back as a CUDA tensor."""
        P = int(n_populations)
        try:
            db = np.ascontiguousarray(np.broadcast_to(np.asarray(dbeta, np.float64), (max(P, 0),)))
        except ValueError:
            raise AnnealingError("dbeta must be a number or hold one entry per population") from None
        rnd = self.counters()[1] if round is None else int(round)
        N_ = self.R // P if P > 0 and self.R % P == 0 else 0
        on_device = _is_tensor(parents)
        if on_device:
            if not parents.is_cuda or parents.dtype != torch.int32 or parents.numel() != self.R or not parents.is_contiguous():
                raise AnnealingError(f"parents must be True, False or a contiguous int32 CUDA tensor of {self.R} entries")
            shift = torch.zeros(max(P, 1), dtype=torch.float64, device=parents.device)
            wsum = torch.zeros(max(P, 1), dtype=torch.int64, device=parents.device)
            if not self.shares_torch_stream():
                _producer_done(parents)
            pp, sp, wp = C.c_void_p(parents.data_ptr()), C.c_void_p(shift.data_ptr()), C.c_void_p(wsum.data_ptr())
            res = parents
        else:
            res = np.zeros(self.R, np.int32) if parents else None
            shift, wsum = np.zeros(max(P, 1), np.float64), np.zeros(max(P, 1), np.uint64)
            pp = None if res is None else res.ctypes.data_as(C.c_void_p)
            sp, wp = shift.ctypes.data_as(C.c_void_p), wsum.ctypes.data_as(C.c_void_p)
        N.check(self._lib.sga_resample(self._h, P, db.ctypes.data_as(C.c_void_p), rnd & 0xFFFFFFFF, pp, sp, wp), "sga_resample")
        if on_device:
            self._observable_done(True)
            self._pending = (res, shift, wsum)
            w = wsum.to(torch.float64)
            w = torch.where(w < 0, w + 2.0 ** 64, w)  # (S up to 2^63 as an unsigned word)
            return res, shift + torch.log(w / (N_ * 2.0 ** 40))
        return res, resample_log_q(shift, wsum, N_)

    # ------------------------------------------------------------------ state access
    def energies(self) -> np.ndarray:
        out = np.zeros(self.R, np.float64)
        N.check(self._lib.sga_get_energies(self._h, out.ctypes.data_as(C.c_void_p)),
                "sga_get_energies")
        return out

    def energies_into(self, tensor, stream_ordered: bool = False):
        """Copy the local energies into a float64 torch tensor (device-to-device on the GPU).  With
        stream_ordered=True (device tensors only) the copy is only enqueued on the engine's stream."""
        if tensor.dtype != torch.float64 or tensor.numel() != self.R or not tensor.is_contiguous():
            raise AnnealingError("need a contiguous float64 tensor of R entries")
        if stream_ordered and tensor.is_cuda:
            N.check(self._lib.sga_get_energies_async(self._h, C.c_void_p(tensor.data_ptr())),
                    "sga_get_energies_async")
        else:
            N.check(self._lib.sga_get_energies(self._h, C.c_void_p(tensor.data_ptr())),
                    "sga_get_energies")
        return tensor

    def temperatures(self) -> np.ndarray:
        out = np.zeros(self.R, np.float64)
        N.check(self._lib.sga_get_temperatures(self._h, out.ctypes.data_as(C.c_void_p)),
                "sga_get_temperatures")
        return out

    def spins(self, r: Optional[int] = None) -> np.ndarray:
        if r is None:
            out = np.zeros((self.R, self.n), np.int8)
            N.check(self._lib.sga_get_spins(self._h, -1, out.ctypes.data_as(C.c_void_p)),
                    "sga_get_spins")
            return out
        out = np.zeros(self._replica_n(r), np.int8)
        N.check(self._lib.sga_get_spins(self._h, int(r), out.ctypes.data_as(C.c_void_p)),
                "sga_get_spins")
        return out

    def set_spins(self, r: int, s):
        a = np.ascontiguousarray(s, dtype=np.int8)
        if a.size != self._replica_n(r):
            raise AnnealingError("spins must have n entries (ragged batches: the replica's model's n)")
        N.check(self._lib.sga_set_spins(self._h, int(r), a.ctypes.data_as(C.c_void_p)),
                "sga_set_spins")

    def best(self, r: Optional[int] = None, with_spins: bool = True):
        """(energy, spins int8 [n] | None, local replica index)."""
        e, idx = C.c_double(0.0), C.c_int(0)
        s = np.zeros(self.n, np.int8) if with_spins else None
        N.check(self._lib.sga_get_best(self._h, -1 if r is None else int(r), C.byref(e),
                                       None if s is None else s.ctypes.data_as(C.c_void_p),
                                       C.byref(idx)), "sga_get_best")
        if s is not None:
            s = s[:self._replica_n(idx.value)].copy() if s.size != self._replica_n(idx.value) else s
        return float(e.value), s, int(idx.value)

    def reset_best(self):
        N.check(self._lib.sga_reset_best(self._h), "sga_reset_best")

    def stats(self):
        acc, att = np.zeros(self.R, np.int64), np.zeros(self.R, np.int64)
        N.check(self._lib.sga_get_stats(self._h, acc.ctypes.data_as(C.c_void_p),
                                        att.ctypes.data_as(C.c_void_p)), "sga_get_stats")
        return acc, att

    def snapshot(self, slots: bool = True):
        """(energies, accepted counters, ladder permutation | None) with one synchronisation."""
        en, acc = np.zeros(self.R, np.float64), np.zeros(self.R, np.int64)
        sm = np.zeros(self.R_global, np.int32) if (slots and self.n_ladders > 0) else None
        N.check(self._lib.sga_snapshot(self._h, en.ctypes.data_as(C.c_void_p), acc.ctypes.data_as(C.c_void_p),
                                       None if sm is None else sm.ctypes.data_as(C.c_void_p)), "sga_snapshot")
        return en, acc, sm

    def slot_map(self) -> np.ndarray:
        out = np.zeros(self.R_global, np.int32)
        N.check(self._lib.sga_get_slot_map(self._h, out.ctypes.data_as(C.c_void_p)),
                "sga_get_slot_map")
        return out

    # ------------------------------------------------------------------ replica observables
    # One exact integer product on the matrix cores (csrc/observables.hip): read only, stream ordered behind the sweeps.
    _WHICH = {"current": N.SPINS_CURRENT, "best": N.SPINS_BEST, N.SPINS_CURRENT: N.SPINS_CURRENT, N.SPINS_BEST: N.SPINS_BEST}

    def _which(self, which) -> int:
        if isinstance(which, (str, int)) and which in self._WHICH:
            return self._WHICH[which]
        raise AnnealingError(f'which must be "current" or "best", not {which!r}')

    def _observable_out(self, out, cols: int):
        """(pointer, ldq, result, device?) for an [R, cols] int32 result: a fresh numpy array, or the caller's CUDA
        tensor (rows may be strided: ldq = out.stride(0)) -- ordered as _buf(..., ordered=True) orders an input."""
        if out is None:
            res = np.zeros((self.R, cols), np.int32)
            return res.ctypes.data_as(C.c_void_p), cols, res, False
        if not _is_tensor(out) or not out.is_cuda or out.dtype != torch.int32 or tuple(out.shape) != (self.R, cols):
            raise AnnealingError(f"out must be an int32 CUDA tensor of shape [{self.R}, {cols}]")
        ldq = int(out.stride(0)) if self.R > 1 else cols  # (one row: its stride is never used)
        if (cols > 1 and out.stride(1) != 1) or ldq < cols:
            raise AnnealingError("out must have unit column stride and rows that do not overlap")
        if not self.shares_torch_stream():
            _producer_done(out)
        return C.c_void_p(out.data_ptr()), ldq, out, True

    def _observable_done(self, device: bool):
        """A device result is only enqueued (as sga_get_energies_async): torch work on another stream waits here."""
        if device and not self.shares_torch_stream():
            N.check(self._lib.sga_snapshot(self._h, None, None, None), "sga_snapshot")  # nothing asked for: the stream's wait

    def magnetizations(self, which="current") -> np.ndarray:
        """int32 [R]: sum_i s_r[i] of every local replica (sga_get_magnetizations; ragged batches: over the model's own
        sites).  which: "current" | "best"."""
        w = self._which(which)
        out = np.zeros(self.R, np.int32)
        N.check(self._lib.sga_get_magnetizations(self._h, w, out.ctypes.data_as(C.c_void_p)), "sga_get_magnetizations")
        return out

    def overlaps(self, which_a="current", which_b=None, out=None):
        """int32 [R, R]: Q[a, b] = sum_i A_a[i] B_b[i] over the local replicas (sga_get_overlaps), A = which_a and B =
        which_b ("current" | "best"; which_b None: which_a) -- n times the overlap q_ab.  out: an optional int32 CUDA
        tensor [R, R] (rows may be strided) that receives the result on the device; with shares_torch_stream() the call
        is only enqueued.  Ragged batches: a pair across models is the dot over the shorter model's sites, meaningless."""
        wa = self._which(which_a)
        wb = wa if which_b is None else self._which(which_b)
        ptr, ldq, res, dev = self._observable_out(out, self.R)
        N.check(self._lib.sga_get_overlaps(self._h, wa, wb, ptr, ldq), "sga_get_overlaps")
        self._observable_done(dev)
        return res

    def overlaps_with(self, configs, which="current", out=None):
        """int32 [R, C]: the local replicas against C configurations of the caller's (sga_get_overlaps_with): configs a
        numpy or torch int8 array [C, n] (a device tensor is read in place, rows may be strided), normally +-1, a 0
        leaves a site out.  One row of ones gives the magnetisations.  out: as in overlaps()."""
        w = self._which(which)
        if _is_tensor(configs):
            t = configs.detach()
            if t.dim() != 2 or t.shape[1] != self.n:
                raise AnnealingError("configs must be [C, n] int8")
            if t.dtype != torch.int8:
                t = t.to(torch.int8)
            if (self.n > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < self.n):
                t = t.contiguous()  # (anything else: rows of a wider tensor pass as they lie, ld = stride(0))
            if not (t.is_cuda and self.shares_torch_stream()):
                _producer_done(t)
            count, ld, cp, keep = int(t.shape[0]), (int(t.stride(0)) if t.shape[0] > 1 else self.n), C.c_void_p(t.data_ptr()), t
        else:
            a = np.asarray(configs)
            if a.ndim != 2 or a.shape[1] != self.n:
                raise AnnealingError("configs must be [C, n] int8")
            if a.dtype != np.int8 or a.strides[1] != 1 or a.strides[0] < self.n:  # (rows of a wider array pass as they lie)
                a = np.ascontiguousarray(a, dtype=np.int8)
            count, ld, cp, keep = int(a.shape[0]), (int(a.strides[0]) if a.shape[0] > 1 else self.n), C.c_void_p(a.ctypes.data), a
        ptr, ldq, res, dev = self._observable_out(out, count)
        N.check(self._lib.sga_get_overlaps_with(self._h, w, cp, ld, count, ptr, ldq), "sga_get_overlaps_with")
        self._observable_done(dev)
        if dev:
            self._pending = (keep, res)  # a converted device operand stays alive while the kernel is queued
        return res

    # ------------------------------------------------------------------ spin and link overlaps between pairs
    # csrc/pair_overlaps.hip: exact integer counts per pair -- d differing sites (n q = n - 2 d), b broken links
    # (L q_l = L - 2 b) over the stored rows -- read only, stream ordered behind the sweeps.
    def link_count(self) -> int:
        """L: the links of the stored rows (sga_get_link_count) -- entries with a value that is not +-0, j != i, both
        triangles as stored.  Sparse (CSR) couplings only."""
        out = np.zeros(1, np.int64)
        N.check(self._lib.sga_get_link_count(self._h, out.ctypes.data_as(C.c_void_p)), "sga_get_link_count")
        return int(out[0])

    def _pair_out(self, out, count: int, dtype, what):
        """(pointer, result, device?) of one output of pair_overlaps: None a fresh numpy array, else the caller's
        contiguous CUDA tensor of `count` entries (ordered as overlaps(out=) orders its tensor)."""
        if out is None:
            res = np.zeros(count, np.int32 if dtype == "int32" else np.int64)
            return res.ctypes.data_as(C.c_void_p), res, False
        if not _is_tensor(out) or not out.is_cuda or out.dtype != getattr(torch, dtype) or out.numel() != count or \
                not out.is_contiguous():
            raise AnnealingError(f"{what} must be a contiguous {dtype} CUDA tensor of {count} entries")
        if not self.shares_torch_stream():
            _producer_done(out)
        return C.c_void_p(out.data_ptr()), out, True

    def pair_overlaps(self, pairs, which="current", links=True, dist=None, broken=None):
        """(dist int32 [count], broken int64 [count] | None) of the pairs (a, b) of LOCAL replica indices
        (sga_get_pair_overlaps): dist the sites where the two differ, broken the links whose two ends differ in that
        (links=False: None, and every kind of problem is served).  Any list: a replica may stand in many pairs, a == b
        gives zeros.  which: "current" | "best".  dist / broken: optional CUDA tensors (int32 / int64, `count` entries)
        that receive the results on the device; with shares_torch_stream() the call is then only enqueued."""
        w = self._which(which)
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        dp, dres, ddev = self._pair_out(dist, len(pr), "int32", "dist")
        bp, bres, bdev = (None, None, False)
        if links:
            bp, bres, bdev = self._pair_out(broken, len(pr), "int64", "broken")
        elif broken is not None:
            raise AnnealingError("broken was given with links=False")
        N.check(self._lib.sga_get_pair_overlaps(self._h, w, pr.ctypes.data_as(C.c_void_p), len(pr), dp, bp), "sga_get_pair_overlaps")
        self._observable_done(ddev or bdev)
        if ddev or bdev:
            self._pending = (pr, dres, bres)  # device results stay alive while the work is queued
        return dres, bres

    def _hist(self, hist, cells, what):
        if not _is_tensor(hist) or not hist.is_cuda or hist.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)) or \
                hist.dim() != 3 or tuple(hist.shape[:2]) != cells or not hist.is_contiguous():
            raise AnnealingError(f"{what} must be a contiguous uint64 or int64 CUDA tensor of shape [{cells[0]}, {cells[1]}, bins]")
        if not self.shares_torch_stream():
            _producer_done(hist)
        return C.c_void_p(hist.data_ptr()), int(hist.shape[2])

    def accumulate_ladder_overlaps(self, hist_q, hist_l=None, slot_lo: int = 0, slot_hi: Optional[int] = None,
                                   q_shift: int = 0, l_shift: int = 0):
        """One count per slot slot_lo <= s < slot_hi (None: every slot) and pair of ladders 2c, 2c + 1 into the caller's
        histograms on the device (sga_accumulate_ladder_overlaps): between the replicas that hold slot s of both now --
        read from the slot map on the device -- bin min(d >> q_shift, bins - 1) of hist_q[c, s - slot_lo] grows by one,
        and, where hist_l is given (sparse couplings), bin min(b >> l_shift, bins - 1) of hist_l[c, s - slot_lo].
        hist_q, hist_l: uint64 or int64 CUDA tensors [n_ladders / 2, slot_hi - slot_lo, bins], zeroed by the caller once;
        the exact layout is shift 0 with n + 1 (link_count() + 1) bins.  Only enqueued: nothing comes back."""
        if self.n_ladders <= 0:
            raise AnnealingError("no ladder (call set_ladder)")
        L = self.R_global // self.n_ladders
        lo, hi = int(slot_lo), L if slot_hi is None else int(slot_hi)
        cells = (self.n_ladders // 2, max(hi - lo, 0))
        qp, bins_q = self._hist(hist_q, cells, "hist_q")
        lp, bins_l = (None, 0) if hist_l is None else self._hist(hist_l, cells, "hist_l")
        N.check(self._lib.sga_accumulate_ladder_overlaps(self._h, lo, hi, qp, bins_q, int(q_shift), lp, bins_l, int(l_shift)),
                "sga_accumulate_ladder_overlaps")
        self._observable_done(True)
        self._pending = (hist_q, hist_l)

    # ------------------------------------------------------------------ class-resolved overlaps between pairs
    # csrc/class_overlaps.hip: per pair and class map, D[m][c] = the differing sites of class c (Q_c = N_c - 2 D_c) as
    # exact integer counts -- read only, stream ordered behind the sweeps.
    def _class_map(self, classes, device_only: bool):
        """(pointer, ld, n_maps, keepalive) of a class map: a numpy array or an int32 CUDA tensor [n_maps, n], or [n]."""
        if _is_tensor(classes) and classes.is_cuda:
            t = classes.reshape(1, -1) if classes.dim() == 1 else classes
            if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] < self.n or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < self.n):
                raise AnnealingError(f"classes must be an int32 CUDA tensor [n_maps, n] or [n] with n = {self.n}, rows contiguous")
            if not self.shares_torch_stream():
                _producer_done(t)
            return C.c_void_p(t.data_ptr()), int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1]), int(t.shape[0]), t
        if device_only:
            raise AnnealingError("classes must be an int32 CUDA tensor (the map stays on the device for the whole run)")
        a = np.asarray(classes.cpu() if _is_tensor(classes) else classes)
        a = np.ascontiguousarray(a.reshape(1, -1) if a.ndim == 1 else a, dtype=np.int32)
        if a.ndim != 2 or a.shape[1] < self.n:
            raise AnnealingError(f"classes must be an array [n_maps, n] or [n] with n = {self.n}")
        return a.ctypes.data_as(C.c_void_p), int(a.shape[1]), int(a.shape[0]), a

    def class_overlaps(self, pairs, classes, n_classes: int, which="current", out=None):
        """int32 [count, n_maps, n_classes]: D[p, m, c], the sites of class c in map m where the two replicas of pair p
        differ (sga_get_class_overlaps); the class overlap is Q_c = N_c - 2 D_c.  pairs: (a, b) of LOCAL replica indices,
        any list, a == b gives zeros.  classes: a numpy array or an int32 CUDA tensor [n_maps, n], or [n]; a value outside
        [0, n_classes) puts the site in no class.  A numpy map is staged on every call: a run keeps its map on the
        device.  which: "current" | "best".  out: an optional contiguous int32 CUDA tensor of that shape that receives the
        result on the device; with shares_torch_stream() the call is then only enqueued."""
        w = self._which(which)
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        cp, ld, n_maps, keep = self._class_map(classes, False)
        shape = (len(pr), n_maps, int(n_classes))
        if out is None:
            res = np.zeros((len(pr), n_maps, max(int(n_classes), 0)), np.int32)
            op, dev = res.ctypes.data_as(C.c_void_p), False
        else:
            if not _is_tensor(out) or not out.is_cuda or out.dtype != torch.int32 or tuple(out.shape) != shape or not out.is_contiguous():
                raise AnnealingError(f"out must be a contiguous int32 CUDA tensor of shape {list(shape)}")
            if not self.shares_torch_stream():
                _producer_done(out)
            res, op, dev = out, C.c_void_p(out.data_ptr()), True
        N.check(self._lib.sga_get_class_overlaps(self._h, w, pr.ctypes.data_as(C.c_void_p), len(pr), cp, ld, n_maps, int(n_classes), op),
                "sga_get_class_overlaps")
        self._observable_done(dev)
        if dev:
            self._pending = (pr, keep, res)  # operands and a device result stay alive while the work is queued
        return res

    def _class_sums(self, t, shape, what):
        if not _is_tensor(t) or not t.is_cuda or t.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)) or \
                tuple(t.shape) != shape or not t.is_contiguous():
            raise AnnealingError(f"{what} must be a contiguous uint64 or int64 CUDA tensor of shape {list(shape)}")
        if not self.shares_torch_stream():
            _producer_done(t)
        return C.c_void_p(t.data_ptr())

    def accumulate_ladder_class_overlaps(self, classes, n_classes: int, sum1, sum2=None, slot_lo: int = 0,
                                         slot_hi: Optional[int] = None):
        """One measurement per slot slot_lo <= s < slot_hi (None: every slot) and pair of ladders 2p, 2p + 1 into the
        caller's sums on the device (sga_accumulate_ladder_class_overlaps): between the replicas that hold slot s of both
        now -- read from the slot map on the device -- D[m, c] is added to sum1[p, s - slot_lo, m, c] and, where sum2 is
        given, D[m, c] D[m, c'] to sum2[p, s - slot_lo, m, c, c'].  classes: an int32 CUDA tensor [n_maps, n] or [n];
        sum1, sum2: uint64 or int64 CUDA tensors [n_ladders / 2, slot_hi - slot_lo, n_maps, n_classes(, n_classes)],
        zeroed by the caller once.  The caller counts its calls.  Only enqueued: nothing comes back."""
        if self.n_ladders <= 0:
            raise AnnealingError("no ladder (call set_ladder)")
        L = self.R_global // self.n_ladders
        lo, hi = int(slot_lo), L if slot_hi is None else int(slot_hi)
        cp, ld, n_maps, keep = self._class_map(classes, True)
        cells = (self.n_ladders // 2, max(hi - lo, 0), n_maps, int(n_classes))
        p1 = self._class_sums(sum1, cells, "sum1")
        p2 = None if sum2 is None else self._class_sums(sum2, cells + (int(n_classes),), "sum2")
        N.check(self._lib.sga_accumulate_ladder_class_overlaps(self._h, lo, hi, cp, ld, n_maps, int(n_classes), p1, p2),
                "sga_accumulate_ladder_class_overlaps")
        self._observable_done(True)
        self._pending = (keep, sum1, sum2)

    def hamming(self, which_a="current", which_b=None) -> np.ndarray:
        """int32 [R, R]: Hamming distances (n_r - Q) / 2 between the configurations of overlaps(which_a, which_b), n_r the
        ROW replica's model size on ragged engines (a pair across models is meaningless there)."""
        Q = self.overlaps(which_a, which_b)
        n_r = np.asarray([self._replica_n(r) for r in range(self.R)], np.int32)
        return ((n_r[:, None] - Q) // 2).astype(np.int32)

    def distinct_best(self, k: int, min_hamming: int = 1, up_to_global_flip: bool = False):
        """Up to k best configurations that are genuinely different: [(replica, energy, spins)].  The replicas are walked
        by best energy ascending (ties by replica index); one is kept when its best configuration is at least
        min_hamming away from every one kept so far -- with up_to_global_flip the distance is (n - |Q|) / 2, for h = 0
        where s and -s are one solution.  Batch engines: distances inside one model only (another model's solutions
        never exclude one).  Costs one overlaps("best", "best"), the best energies (read replica by replica: sga_get_best
        has no bulk form) and one best(r) read per configuration returned."""
        Q = self.overlaps("best", "best").astype(np.int64)
        energy = np.asarray([self.best(r, with_spins=False)[0] for r in range(self.R)]) if self.R else np.zeros(0)
        model = [(self.replica0 + r) // max(self.R_global // max(self.n_models, 1), 1) for r in range(self.R)]
        kept = []
        for r in sorted(range(self.R), key=lambda i: (energy[i], i)):
            if len(kept) >= int(k):
                break
            n_r = self._replica_n(r)
            q = np.abs(Q[r]) if up_to_global_flip else Q[r]
            if all(model[j] != model[r] or (n_r - q[j]) // 2 >= int(min_hamming) for j in kept):
                kept.append(r)
        return [(r, float(energy[r]), self.best(r)[1]) for r in kept]

    def route_query(self):
        """The query the engine itself poses to the form selection (sga_get_route_query)."""
        q = N.RouteQuery()
        N.check(self._lib.sga_get_route_query(self._h, C.byref(q)), "sga_get_route_query")
        return q

    def scan_summary(self, model: int = 0):
        """(kind, words) the set-time scans wrote for the problem as held (sga_get_scan_summary; layout in include/sga.h):
        kind N.ROUTE_DENSE with 8 words -- a dense batch is scanned stacked, model must be 0 -- or N.ROUTE_CSR with the
        CSR words and the longest row, per model of a ragged batch."""
        kind, count = C.c_int32(-1), C.c_int(0)
        words = (C.c_int32 * 16)()
        N.check(self._lib.sga_get_scan_summary(self._h, int(model), C.byref(kind), words, 16, C.byref(count)),
                "sga_get_scan_summary")
        return int(kind.value), [int(w) for w in words[:count.value]]

    def explain_route(self) -> str:
        """What csrc/sga_route.cpp answers for this engine's problem, replicas and options."""
        return N.explain_route(self.route_query())

    def last_kernel(self) -> str:
        """The kernel instantiation THIS engine's last sweep launched (sga_get_last_kernel; per engine, so that two
        engines on two threads do not see each other's)."""
        buf = C.create_string_buffer(512)
        N.check(self._lib.sga_get_last_kernel(self._h, buf, 512), "sga_get_last_kernel")
        return buf.value.decode()

    def exchange_stats(self):
        a, b = np.zeros(self.R_global, np.int64), np.zeros(self.R_global, np.int64)
        N.check(self._lib.sga_get_exchange_stats(self._h, a.ctypes.data_as(C.c_void_p),
                                                 b.ctypes.data_as(C.c_void_p)),
                "sga_get_exchange_stats")
        return a, b

    def counters(self):
        s, r = C.c_uint32(0), C.c_uint32(0)
        N.check(self._lib.sga_get_sweep_counter(self._h, C.byref(s), C.byref(r)))
        return int(s.value), int(r.value)

    def set_seed(self, seed: int):
        N.check(self._lib.sga_set_seed(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_counters(self, sweeps_done: int, exchange_rounds: int):
        N.check(self._lib.sga_set_sweep_counter(self._h, int(sweeps_done), int(exchange_rounds)))

    # ------------------------------------------------------------------ checkpoint / resume
    def export_state(self) -> bytes:
        """Everything needed to continue this run bit-exactly (see sga_export_state)."""
        need = C.c_uint64(0)
        N.check(self._lib.sga_export_state(self._h, None, 0, C.byref(need)), "sga_export_state")
        buf = (C.c_ubyte * need.value)()
        N.check(self._lib.sga_export_state(self._h, buf, need.value, None), "sga_export_state")
        return bytes(buf)

    def import_state(self, blob: bytes):
        buf = (C.c_ubyte * len(blob)).from_buffer_copy(blob)
        N.check(self._lib.sga_import_state(self._h, buf, len(blob)), "sga_import_state")

    # ------------------------------------------------------------------ measurement
    def enable_timing(self, on: bool = True):
        N.check(self._lib.sga_enable_timing(self._h, 1 if on else 0))

    def kernel_time(self, reset: bool = True):
        """(launches, total_ms) of the sweep-kernel launches since the last reset."""
        n, ms = C.c_int64(0), C.c_double(0.0)
        N.check(self._lib.sga_get_kernel_time(self._h, C.byref(n), C.byref(ms), 1 if reset else 0))
        return int(n.value), float(ms.value)

    def describe(self) -> str:
        buf = C.create_string_buffer(512)
        N.check(self._lib.sga_describe(self._h, buf, 512))
        return buf.value.decode()


def option_names():
    """Every key sga_set_option accepts."""
    names, buf = [], C.create_string_buffer(64)
    while N.lib().sga_option_name(len(names), buf, 64) == N.OK:
        names.append(buf.value.decode())
    return names


def last_kernel() -> str:
    """The kernel instantiation this thread's last sweep launched (sga_last_kernel)."""
    buf = C.create_string_buffer(256)
    N.check(N.lib().sga_last_kernel(buf, 256), "sga_last_kernel")
    return buf.value.decode()


def op_pt_exchange(device: int, spins, energies, temps, u=None, seed: int = 0, round_: int = 0):
    """Operator-form PT exchange on fp32 buffers, in place (reference cuda_kernels.py:415-443)."""
    lib = N.lib()
    sp, k1 = _buf(spins, np.float32, "float32")
    ep, k2 = _buf(energies, np.float32, "float32")
    tp, k3 = _buf(temps, np.float32, "float32")
    up, k4 = _buf(u, np.float32, "float32")
    if _is_tensor(spins):
        if k1.data_ptr() != spins.data_ptr() or k2.data_ptr() != energies.data_ptr():
            raise AnnealingError("spins/energies must be contiguous float32 (updated in place)")
        R, n = spins.shape
    else:
        if k1 is not spins or k2 is not energies:
            raise AnnealingError("spins/energies must be contiguous float32 (updated in place)")
        R, n = k1.shape
    out = C.c_int(0)
    N.check(lib.sga_op_pt_exchange(int(device), sp, ep, tp, up, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                   int(round_), int(R), int(n), C.byref(out)), "sga_op_pt_exchange")
    return int(out.value)
