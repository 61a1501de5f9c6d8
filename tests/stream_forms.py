"""One table of forced sweep forms, and the two chains the stream-coordinate tests compare (test infrastructure).

Every result of the engine is the oracle's chain, and that chain is defined by four Philox coordinates: the 64-bit seed,
the sweep counter (uint32, wraps at 2^32), the GLOBAL replica id and the update index inside a sweep.  Each sweep form
builds these coordinates for itself, so each form is an entry here: a small problem, the options that force the form,
a predicate on last_kernel() / describe() proving that it ran, and the source files whose philox4x32_10 call sites it
reaches (tests/test_stream_coordinates_host.py checks that no such file is left without a form).  The problems, option
sets and predicates are those of the per-form test files; they are imported, not restated.

OracleChain walks global replicas [g0, g0 + R) of a set of R_global on the CPU oracle; EngineChain drives an engine
shard of the same replicas.  Both return the same state dictionary."""
import functools

import numpy as np

import oracle

MASK32 = 0xFFFFFFFF
ENGINE_FILES = ("sga_misc.hip",)  # every form draws its initial spins there (init_replicas with s0 = None)


def _te():
    import test_temperature_edges_gpu as m
    return m


class Built:
    """What a form's builder returns: the models (one oracle.Problem, or one per model of a batch), setup(engine),
    want(last_kernel, describe) and the temperature range (hot, cold) that keeps both accepts and rejects in play."""

    def __init__(self, models, setup, want, trange):
        self.models = models if isinstance(models, (list, tuple)) else [models]
        self.setup, self.want, self.trange = setup, want, trange


class Form:
    def __init__(self, name, files, builder, exact=True, rule=0, site_mode=0, recompute=False, R_global=100, R_small=8,
                 plan=(2, 3), want_last_only=False, single=True):
        self.name, self.files, self._builder = name, tuple(files) + ENGINE_FILES, builder
        self.exact, self.rule, self.site_mode, self.recompute = exact, rule, site_mode, recompute
        self.R_global, self.R_small, self.plan = R_global, R_small, tuple(plan)
        self.want_last_only, self.single = want_last_only, single

    @functools.lru_cache(maxsize=None)
    def build(self):
        return self._builder()

    def __repr__(self):
        return self.name


def temps_for(b, R_global):
    """Temperature of global replica g: eight values from hot to cold, cycling with g, so that every shard of eight or
    more replicas holds hot and cold replicas whatever its cut."""
    hot, cold = b.trange
    return np.asarray([hot * (cold / hot) ** ((g % 8) / 7.0) for g in range(R_global)], np.float64)


def ladder_for(b, R):
    hot, cold = b.trange
    return np.asarray([hot * (cold / hot) ** (i / max(R - 1, 1)) for i in range(R)], np.float64)


# ----------------------------------------------------------------------------- builders
def _fields(n, seed, lo=-1, hi=1, div=1.0):
    return (np.random.RandomState(seed).randint(lo, hi + 1, n) / div).astype(np.float32)


def dense_streaming(storage, look, n=256):
    def build():
        te = _te()
        J, h = te.pm1(n, 3), _fields(n, 4)

        def setup(e):
            e.set_options({} if look else {"look_ahead": 0})
            e.set_dense(J, h, storage=storage)

        def want(k, d):
            la = "look_ahead=4" in d or "look_ahead=2" in d
            return k.startswith("sweep_dense_kernel") and f"storage={storage}" in d and la == look
        return Built(oracle.Problem(J=J, h=h), setup, want, (3.0 * np.sqrt(n), 0.1 * np.sqrt(n)))
    return build


def dense_general(site_mode):
    """force_general, and sequential sites without recorded uniforms (Philox uniforms): the general builds."""
    def build():
        te, n = _te(), 200
        J, h = te.pm1(n, 7), _fields(n, 7)

        def setup(e):
            if not site_mode:
                e.set_options(force_general=1)
            e.set_dense(J, h, storage="f32")
        return Built(oracle.Problem(J=J, h=h), setup,
                     lambda k, d: k.startswith("sweep_dense_kernel") and "LEAN=0" in k, (40.0, 1.5))
    return build


def dense_fp64(canonical):
    def build():
        n, rng = 200, np.random.RandomState(8)
        if canonical:
            J = np.triu(rng.randn(n, n), 1).astype(np.float32)
            J, h = J + J.T, rng.randn(n).astype(np.float32)

            def setup(e):
                e.set_options(force_dense_canonical=1)
                e.set_dense(J, h)
            return Built(oracle.Problem(J=J, h=h), setup,
                         lambda k, d: "acc=f64-canonical" in d and "CANON=1" in k, (30.0, 1.0))
        J = np.triu(rng.randint(-30000, 30001, (n, n)), 1).astype(np.float32)
        J, h = (J + J.T) * 4096.0, rng.randint(-500, 501, n).astype(np.float32)
        return Built(oracle.Problem(J=J, h=h), lambda e: e.set_dense(J, h),
                     lambda k, d: "acc=f64" in d and "ACC64=1" in k, (1.2e9, 4e7))
    return build


def dense_rule(rule):
    def build():
        te, n = _te(), 200
        J, h = te.int_couplings(n, 5, 2, density=0.1), _fields(n, 5, -2, 2)
        return Built(oracle.Problem(J=J, h=h), lambda e: (e.set_options(sparse_route=0), e.set_dense(J, h, storage="f32")),
                     lambda k, d: k.startswith("sweep_dense_kernel") and "storage=f32" in d, (12.0, 0.4))
    return build


def csr_rule(rule):
    def build():
        te, n = _te(), 200
        J, h = te.int_couplings(n, 5, 2, density=0.1), _fields(n, 5, -2, 2)
        csr = te.csr_of(J)
        return Built(oracle.Problem(csr=csr, h=h), lambda e: e.set_csr(*csr, h), lambda k, d: k.startswith("sweep_csr"),
                     (12.0, 0.4))
    return build


def row_shared(n, W, storage, kind, source):
    def build():
        import test_row_shared_planes_gpu as rs
        J, h = rs.couplings(n, kind, 17 + n), rs.fields(n, kind, n)
        amp = {"pm1": 1, "tern": 1, "a7": 7, "a100": 100}[kind]

        def setup(e):
            rs.forced(e, W)
            e.set_dense(J, h, storage=storage)

        def want(k, d):
            return (f"sweep=row-shared(W={W} planes=" in d and k.startswith("sweep_dense_rs<")
                    and f"fields from {source}" in k)
        return Built(oracle.Problem(J=J, h=h), setup, want, (2.0 * amp * np.sqrt(n), 0.3))
    return build


def dense_cached(batched=None, waves=0, wide=False, half_h=False):
    def build():
        te = _te()
        n = 1100 if waves else 600
        if wide:
            n = 700
            J, h, storage = te.int_couplings(n, 12, 120, density=0.9), _fields(n, 12, -120, 120), "i8"
            trange = (120.0 * 3.0 * np.sqrt(n), 120.0)
        else:
            J, storage = te.pm1(n, 6), "auto"
            h = _fields(n, 6, -2, 2, 2.0) if half_h else _fields(n, 6)
            trange = (3.0 * np.sqrt(n), 0.1 * np.sqrt(n))
        name = "sweep_clf" if batched is None else "sweep_clfb_kernel" if batched else "sweep_clf_kernel"
        bits = 32 if wide else 16

        def setup(e):
            if batched is not None:
                e.set_options(clf_batched=batched)
            if waves:
                e.set_options(clf_waves=waves)
            e.set_field_cache("on")
            e.set_dense(J, h, storage=storage)

        def want(k, d):
            return (k.startswith(name) and f"sweep=cached-local-fields(int{bits}" in d and f"int{bits}_t" in k
                    and (not waves or f"x {waves} wave" in k) and (batched != 0 or waves or "LEAN" in k))
        return Built(oracle.Problem(J=J, h=h), setup, want, trange)
    return build


def dense_fixed_point(bits):
    def build():
        import test_dense_fixed_point_gpu as fx
        if bits == 32:
            n = 400
            J, h, trange = fx.grid_sk(n, 3), (np.random.RandomState(4).randn(n) * 0.7).astype(np.float32), (40.0, 0.3)
        else:  # one coupling of 2^24 beside the 2^-10 grid
            n = 500
            J = fx.grid_sk(n, 5, scale=0.1)
            J[3, 400] = J[400, 3] = np.float32(2.0 ** 24)
            h, trange = (np.random.RandomState(5).randn(n) * 0.3).astype(np.float32), (3.0e7, 0.5)

        def setup(e):
            e.set_option("clf_fixed_point", 1)
            e.set_field_cache("on")
            e.set_dense(J, h)
        return Built(oracle.Problem(J=J, h=h), setup,
                     lambda k, d: k.startswith("sweep_clf_fx_kernel<float") and f"int{bits} fixed-point" in k, trange)
    return build


def dense_auto(fixed_point):
    """SGA_FIELD_CACHE_AUTO with a hot end that stays on the row kernels and a cold end that goes cached: the mixed
    launch over two replica lists."""
    def build():
        import test_dense_fixed_point_gpu as fx
        te, n = _te(), 800
        if fixed_point:
            J, h = fx.grid_sk(n, 16), (np.random.RandomState(9).randn(n) * 0.3).astype(np.float32)
        else:
            J, h = te.pm1(n, 9), np.zeros(n, np.float32)

        def setup(e):
            if fixed_point:
                e.set_option("clf_fixed_point", 1)
            e.set_field_cache("auto")
            e.set_dense(J, h)
        cached = "sweep_clf_fx_kernel" if fixed_point else "sweep_clf"
        return Built(oracle.Problem(J=J, h=h), setup, lambda k, d: k.startswith("mixed launch") and cached in k,
                     (200.0, 0.02) if fixed_point else (6000.0, 0.5))
    return build


def dense_batch(cached):
    def build():
        import test_batch_cached_fields_gpu as bc
        n, M = 96, 3
        Js, hs = bc.pm1_batch(n, M, 200)

        def setup(e):
            e.set_field_cache("on" if cached else "off")
            e.set_dense_batch(Js, hs)

        def want(k, d):
            return f"models={M}" in d and (k.startswith("sweep_clf") if cached else
                                           k.startswith("sweep_dense_kernel") and "BATCH=1" in k)
        return Built([oracle.Problem(J=Js[m], h=hs[m]) for m in range(M)], setup, want, (30.0, 1.0))
    return build


def csr_forms(upd, bits, half_h=False):
    def build():
        te, n = _te(), 400
        J = te.sparse_int(n, 12, 1, 100 + n)
        h = _fields(n, 13, -2, 2, 2.0 if half_h else 1.0)
        csr = te.csr_of(J)

        def setup(e):
            e.set_options(csr_updates_per_step=upd, force_csr_bits=int(bits))
            e.set_csr(*csr, h)

        def want(k, d):
            rows = upd >= 4
            return (("sweep_csr_rows_kernel" in k) == rows and (not rows or f"<{upd} rows" in k)
                    and k.startswith("sweep_csr") and ("bit spins" in k) == bits)
        return Built(oracle.Problem(csr=csr, h=h), setup, want, (12.0, 0.4))
    return build


def csr_real(upd):
    def build():
        te, n, rng = _te(), 300, np.random.RandomState(14)
        J = np.triu((rng.rand(n, n) < 0.04) * rng.randn(n, n), 1).astype(np.float32)
        J, h = J + J.T, rng.randn(n).astype(np.float32)
        csr = te.csr_of(J)

        def setup(e):
            e.set_options(csr_updates_per_step=upd, force_csr_acc=3)
            e.set_csr(*csr, h)
        return Built(oracle.Problem(csr=csr, h=h), setup,
                     lambda k, d: ("fp64 canonical sums" in k) if upd else k.startswith("sweep_csr_kernel<acc=3"), (12.0, 0.4))
    return build


def csr_wide(bits, packed=False):
    def build():
        te, n, rng = _te(), 900, np.random.RandomState(17)
        amp = rng.randint(-127, 128, (n, n)) if packed else (rng.randint(0, 2, (n, n)) * 2 - 1)
        J = (np.triu(rng.rand(n, n) < 0.35, 1) * amp).astype(np.float32)
        J, h = J + J.T, _fields(n, 17, -2, 2)
        csr = te.csr_of(J)

        def setup(e):
            e.set_options(force_csr_bits=int(bits), csr_bits=int(bits))
            e.set_tuning(waves_per_replica=2)
            if packed:
                e.set_csr_storage("packed")
            e.set_csr(*csr, h)

        def want(k, d):
            return ("one replica per workgroup" in k and "waves_per_replica=2" in d and ("bit spins" in k) == bits
                    and (not packed or "entries=packed-32bit" in d))
        scale = 127.0 if packed else 1.0
        return Built(oracle.Problem(csr=csr, h=h), setup, want, (54.0 * scale, 2.0 * scale))
    return build


def csr_cached(bits):
    def build():
        import test_fixed_point_fields_gpu as fx
        te = _te()
        if bits == 16:
            n = 1000
            J, h, trange = te.sparse_int(n, 10, 2, 7), _fields(n, 15, -3, 3), (18.0, 0.6)
            csr = te.csr_of(J)
        elif bits == 32:
            n = 900
            J = fx.sparse_J(n, 14, 3, fx.binary_grid)
            h, trange, csr = (np.random.RandomState(4).randn(n) * 0.7).astype(np.float32), (40.0, 0.1), fx.csr_of(J)
        else:
            csr, h = fx.tsp_instance(24)
            trange = (200.0, 2.0)

        def setup(e):
            if bits != 16:
                e.set_option("clf_fixed_point", 1)
            e.set_field_cache("on")
            e.set_csr(*csr, h)

        def want(k, d):
            return k.startswith("sweep_clf_csr_kernel") and (f"int{bits} fixed-point" in k if bits != 16 else "int16 fields" in k)
        return Built(oracle.Problem(csr=csr, h=h), setup, want, trange)
    return build


def ragged_batch():
    import test_ragged_batch_gpu as rg
    specs = [(3, 1.0, False), (37, 0.3, True), (257, 0.05, False), (1201, 0.007, True)]
    probs = [(*rg.sym_sparse(n, dens, 10 + m), rg.fields(n, 20 + m, half)) for m, (n, dens, half) in enumerate(specs)]
    return Built([oracle.Problem(csr=p[:3], h=p[3]) for p in probs], lambda e: e.set_csr_batch(probs),
                 lambda k, d: "ragged" in k, (12.0, 0.4))


def tsp(par):
    def build():
        from spin_glass_anneal_rl_amd import encoders as enc
        nc = 17
        xy = np.random.RandomState(300 + nc).rand(nc, 2) * 100.0
        dist = np.rint(np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1]) / 4.0) * 4.0
        d32, A, B, h, _ = enc.tsp_structure(dist, 200.0, 120.0, auto_scale=False)
        csr = oracle.tsp_to_csr(d32, A, B)

        def setup(e):
            e.set_options(tsp_updates_per_step=par)
            e.set_tsp(d32, A, B, h)

        def want(k, d):
            return ("sweep_tsp_par_kernel" in k and f"x {par} updates" in k) if par > 1 else k.startswith("sweep_tsp_kernel")
        return Built(oracle.Problem(csr=(csr[0].astype(np.int32), csr[1], csr[2]), h=h), setup, want, (300.0, 10.0))
    return build


def wolff(kind):
    def build():
        te, n = _te(), 120
        J, h = te.int_couplings(n, 16, 2, density=0.05), _fields(n, 16)
        csr = te.csr_of(J)
        if kind == "dense":
            return Built(oracle.Problem(J=J, h=h), lambda e: (e.set_options(sparse_route=0), e.set_dense(J, h)),
                         lambda k, d: d.startswith("dense"), (30.0, 4.0))
        return Built(oracle.Problem(csr=csr, h=h), lambda e: e.set_csr(*csr, h), lambda k, d: d.startswith("csr"), (30.0, 4.0))
    return build


# ----------------------------------------------------------------------------- the table
COMMON, CLF, CLFB = "sweep_common.h", "sweep_clf_impl.h", "sweep_clfb_impl.h"
AUTO_PLAN = (4, 4, 8, 8)

FORMS = (
    # dense, a coupling row per proposal
    [Form(f"dense-{s}-look{int(look)}", [COMMON], dense_streaming(s, look)) for s in ("f32", "i8", "t2") for look in (True, False)]
    + [Form("dense-force-general", [COMMON], dense_general(0)),
       Form("dense-sequential-philox-u", [COMMON], dense_general(1), site_mode=oracle.SITE_SEQUENTIAL),
       Form("dense-f64-exact", [COMMON], dense_fp64(False)),
       Form("dense-f64-canonical", [COMMON], dense_fp64(True), exact=False),
       Form("dense-glauber", [COMMON], dense_rule(1), rule=1), Form("dense-heat-bath", [COMMON], dense_rule(2), rule=2)]
    # dense, row-shared windows (groups of 32 replicas: R = 100 leaves a ragged last group of 4)
    + [Form("row-shared-W256-planes", ["sweep_dense_rs.hip"], row_shared(257, 256, "f32", "pm1", "resident bit-planes"), R_small=34),
       Form("row-shared-W1024-on-chip", ["sweep_dense_rs.hip"], row_shared(520, 1024, "i8", "a100", "on-chip conversion"), R_small=34)]
    # dense, cached local fields
    + [Form("clf-one-accept", [CLF], dense_cached(batched=0)), Form("clfb-several-accepts", [CLFB], dense_cached(batched=1)),
       Form("clf-waves8", [CLF, CLFB], dense_cached(waves=8)),
       Form("clf-int32-fields", [CLF], dense_cached(batched=0, wide=True)), Form("clfb-int32-fields", [CLFB], dense_cached(batched=1, wide=True)),
       Form("clf-half-integer-h", [CLF, CLFB], dense_cached(half_h=True)),
       Form("clf-fixed-point-int32", [COMMON], dense_fixed_point(32)), Form("clf-fixed-point-int64", [COMMON], dense_fixed_point(64)),
       Form("auto-mixed-integer", [COMMON, CLF, CLFB], dense_auto(False), R_global=60, plan=AUTO_PLAN, want_last_only=True),
       Form("auto-mixed-fixed-point", [COMMON], dense_auto(True), R_global=60, plan=AUTO_PLAN, want_last_only=True)]
    # dense batches
    + [Form("dense-batch-rows", [COMMON], dense_batch(False), R_global=102, R_small=9, single=False),
       Form("dense-batch-cached", [CLF, CLFB], dense_batch(True), R_global=102, R_small=9, single=False)]
    # CSR
    + [Form(f"csr-upd{u}", ["sweep_csr_rows.hip" if u >= 4 else COMMON], csr_forms(u, False)) for u in (0, 2, 4, 8)]
    + [Form("csr-force-bits", [COMMON], csr_forms(0, True)), Form("csr-rows4-bits-half-h", ["sweep_csr_rows.hip"], csr_forms(4, True, True)),
       Form("csr-wide-bit-spins", [COMMON], csr_wide(True)), Form("csr-wide-byte-spins", [COMMON], csr_wide(False)),
       Form("csr-packed-entries", [COMMON], csr_wide(True, packed=True)),
       Form("csr-f64-canonical", [COMMON], csr_real(0), exact=False),
       Form("csr-rows4-f64-canonical", ["sweep_csr_rows.hip"], csr_real(4), exact=False),
       Form("csr-cached-int16", ["sweep_clf_csr.hip"], csr_cached(16)),
       Form("csr-fixed-point-int32", ["sweep_clf_csr.hip", COMMON], csr_cached(32)),
       Form("csr-fixed-point-int64", ["sweep_clf_csr.hip", COMMON], csr_cached(64)),
       Form("csr-glauber", [COMMON], csr_rule(1), rule=1), Form("csr-heat-bath", [COMMON], csr_rule(2), rule=2)]
    # the other forms
    + [Form("ragged-csr-batch", [COMMON], ragged_batch, R_small=8, single=False),
       Form("tsp-one-update", [COMMON], tsp(1)), Form("tsp-8-updates", ["sweep_tsp.hip"], tsp(8)),
       Form("wolff-dense", ["sweep_wolff.hip", COMMON], wolff("dense"), rule=oracle.RULE_WOLFF, recompute=True),
       Form("wolff-csr", ["sweep_wolff.hip", COMMON], wolff("csr"), rule=oracle.RULE_WOLFF, recompute=True)]
)
BY_NAME = {f.name: f for f in FORMS}
assert len(BY_NAME) == len(FORMS)


# ----------------------------------------------------------------------------- the two chains
STATE_EXACT = ("spins", "acc", "best_s")
STATE_ENERGY = ("trace", "energy", "best_e")


def assert_same(a, b, exact, tag):
    """Everything a run leaves behind.  exact=False (the canonical-sum forms against the ORACLE only): the energies at
    the tolerance their own test file uses, the chain itself -- spins, accept counters, best spins -- still equal."""
    for key in STATE_EXACT:
        assert len(a[key]) == len(b[key]), (tag, key)
        assert all(np.array_equal(x, y) for x, y in zip(a[key], b[key])), (tag, key)
    for key in STATE_ENERGY:
        if exact:
            assert np.array_equal(a[key], b[key]), (tag, key)
        else:
            assert np.allclose(a[key], b[key], rtol=1e-6, atol=1e-5), (tag, key)


def slice_state(st, lo, hi):
    out = {k: st[k][lo:hi] for k in ("spins", "acc", "best_s", "energy", "best_e")}
    out["trace"] = st["trace"][:, lo:hi]
    return out


class OracleChain:
    """Global replicas [g0, g0 + R) of R_global on the CPU oracle; replica g belongs to model g // (R_global / M)."""

    def __init__(self, form, R_global, g0, R, seed, temps, c0=0):
        b = form.build()
        self.form, self.models, self.seed, self.done = form, b.models, seed, c0 & MASK32
        self.temps = np.asarray(temps, np.float64)
        assert self.temps.shape == (R,) and R_global % len(b.models) == 0
        k = R_global // len(b.models)
        self.parts, r = [], 0
        while r < R:
            m = (g0 + r) // k
            cnt = min(R - r, (m + 1) * k - (g0 + r))
            self.parts.append((m, slice(r, r + cnt), g0 + r))
            r += cnt
        self.spins = [oracle.init_spins(self.models[m].n, sl.stop - sl.start, seed, replica0=g) for m, sl, g in self.parts]
        self.energy = [np.atleast_1d(oracle.energy(self.models[m], s)).astype(np.float64)
                       for (m, _, _), s in zip(self.parts, self.spins)]
        self.best_e = [e.copy() for e in self.energy]
        self.best_s = [s.copy() for s in self.spins]
        self.acc = np.zeros(R, np.int64)
        self.R, self.traces = R, []

    def set_seed(self, seed):
        self.seed = seed

    def sweep(self, ns):
        tr = np.zeros((ns, self.R))
        for i, (m, sl, g) in enumerate(self.parts):
            u = None
            if self.form.site_mode == oracle.SITE_SEQUENTIAL:
                # sequential sites without recorded uniforms take update t's Philox uniform: the oracle is handed its
                # own stream_u as the recorded ones
                n = self.models[m].n
                u = np.asarray([[oracle.stream_u(self.seed, g + r, (self.done + k) & MASK32, t) for k in range(ns)
                                 for t in range(n)] for r in range(sl.stop - sl.start)], np.float32)
            ref = oracle.sweeps(self.models[m], self.spins[i], self.temps[sl], ns, site_mode=self.form.site_mode,
                                replay_u=u, rule=self.form.rule, seed=self.seed, sweep0=self.done, replica0=g, energy=self.energy[i],
                                best_energy=self.best_e[i], recompute_energy=self.form.recompute, n_threads=16)
            better = ref["best_energy"] < self.best_e[i]
            self.best_s[i][better] = ref["best_spins"][better]
            self.best_e[i], self.energy[i] = ref["best_energy"], ref["energy"]
            self.acc[sl] += ref["n_accepted"]
            tr[:, sl] = ref["energy_trace"]
        self.done = (self.done + ns) & MASK32
        self.traces.append(tr)
        return tr

    def state(self):
        return dict(trace=np.vstack(self.traces) if self.traces else np.zeros((0, self.R)), spins=[r for s in self.spins for r in s], acc=self.acc.copy(),
                    energy=np.concatenate(self.energy), best_e=np.concatenate(self.best_e),
                    best_s=[r for s in self.best_s for r in s])


class EngineChain:
    """The same replicas on an engine that is forced onto the form; every sweep call asserts the form's predicate."""

    def __init__(self, sg, form, R_global, g0, R, seed, temps=None, c0=None, init=True):
        b = form.build()
        self.form, self.b, self.R, self.traces, self.kernels = form, b, R, [], []
        self.e = sg.AnnealEngine(0)
        try:
            b.setup(self.e)
            self.e.set_update_rule(form.rule)
            if init:
                self.e.init_replicas(R, seed=seed, R_global=R_global, replica0=g0)
                if temps is not None:
                    self.e.set_temperatures(temps)
                if c0 is not None:
                    self.e.set_counters(c0, 0)
        except BaseException:
            self.e.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.close()

    def sweep(self, ns, last=True):
        tr = self.e.sweep(ns, site_mode=self.form.site_mode, energy_trace=True)["energy_trace"]
        self.note(last)
        self.traces.append(tr)
        return tr

    def note(self, last=True):
        """The form's predicate on what the last sweep launched (AUTO: on a plan's last call, once it has routed)."""
        k, d = self.e.last_kernel(), self.e.describe()
        self.kernels.append(k)
        if last or not self.form.want_last_only:
            assert self.b.want(k, d), (self.form.name, k, d)

    def run(self, plan):
        for i, ns in enumerate(plan):
            self.sweep(ns, last=i + 1 == len(plan))
        return self.state()

    def state(self):
        e, R = self.e, self.R
        best = [e.best(r) for r in range(R)]
        return dict(trace=np.vstack(self.traces) if self.traces else np.zeros((0, R)), spins=[e.spins(r) for r in range(R)],
                    acc=e.stats()[0].copy(), energy=e.energies().copy(), best_e=np.asarray([x[0] for x in best]),
                    best_s=[x[1] for x in best])
