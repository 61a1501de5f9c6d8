"""One engine, many problems: stations, walks and the comparison (test infrastructure; imports without a GPU).

The C ABI lets one engine take any number of problems, and the long-lived callers (IsingModel._engine,
CUDAKernelManager._engine) do exactly that.  What one problem leaves behind for the next is decided by where a member
is declared in csrc/sga_engine_impl.h (ProblemState and ReplicaState are reset whole by free_problem / free_replicas,
what stays in sga_engine survives), so the tests walk ONE engine through problems of every kind and compare every
visit with a FRESH engine given the same settings and the same calls.  Same code, same inputs: everything is equal, no
tolerance.  So that "fresh and re-used are wrong alike" cannot pass, a station's last visit in a walk is also held
against the CPU oracle.

A STATION is a small problem, one per setter and value class; the problems are those of the per-form test files
(stream_forms, groups_cases, groups_rest_cases), imported where a builder exists and rebuilt by the same recipe where
the problem lives inside a test function.  A VISIT is: the caller's settings back to their defaults, the station's own
settings and setter, init_replicas(R, seed), a ladder (or plain temperatures), sweep(2), exchange(), sweep(1), collect.
"""
import functools

import numpy as np

import oracle
import stream_forms as sf
from oracle_engine import OracleEngine

KINDS = ("dense", "batch", "csr", "ragged", "tsp", "groups", "groups_rest")
R_CYCLE = (3, 33, 8)  # sstride, the 32-replica groups, the one-pass energy paths
SEED = 9001


# ----------------------------------------------------------------------------- stations
class Station:
    def __init__(self, sid, kind, builder, exact=True, leaves=""):
        self.id, self.kind, self._builder, self.exact, self.leaves = sid, kind, builder, exact, leaves

    @functools.lru_cache(maxsize=None)
    def build(self):
        return self._builder()

    def __repr__(self):
        return self.id


def _d2():
    te, n = sf._te(), 200
    J, h = te.pm1(n, 21), sf._fields(n, 22, -2, 2, 2.0)
    return sf.Built(oracle.Problem(J=J, h=h), lambda e: (e.set_field_cache("on"), e.set_dense(J, h)), None,
                    (3.0 * np.sqrt(n), 0.1 * np.sqrt(n)))


def _d5():
    """The recipe of test_set_time_scans_gpu.test_dense_matrix_kept_as_csr_reports_the_csr_words (it lives inside the
    test): a sparse integer matrix handed over dense under field cache OFF, n >= 4096, is kept as CSR."""
    te, n = sf._te(), 4097
    rng = np.random.RandomState(9)
    J = np.zeros((n, n), np.float32)
    i, j = rng.randint(0, n, 3 * n), rng.randint(0, n, 3 * n)
    keep = i != j
    J[i[keep], j[keep]] = rng.randint(1, 4, keep.sum())
    J = np.triu(J, 1)
    J = J + J.T
    J[77, :] = J[:, 77] = 0.0  # an empty row
    h = rng.randint(-2, 3, n).astype(np.float32)
    return sf.Built(oracle.Problem(csr=te.csr_of(J), h=h), lambda e: (e.set_field_cache("off"), e.set_dense(J, h)), None,
                    (12.0, 0.4))


def _d6():
    te, n = sf._te(), 300
    J, h = te.int_couplings(n, 23, 1, density=0.6), sf._fields(n, 24)
    return sf.Built(oracle.Problem(J=J, h=h), lambda e: e.set_dense(J, h, storage="t2"), None, (30.0, 1.0))


def _c4():
    """The (301, 9, 5, half-integer h, dups) case of test_engine_gpu.test_csr_pair_look_ahead_equals_one_update_at_a_time
    (it lives inside the test): some entries split into two that add up -- unsorted rows, duplicate columns."""
    te, n, deg, amp = sf._te(), 301, 9, 5
    rng = np.random.RandomState(7 * n + deg)
    J = np.zeros((n, n), np.float32)
    for i in range(n):
        for j in rng.choice(n, min(deg // 2 + 1, n), replace=False):
            if i != j:
                J[i, j] = J[j, i] = float(rng.choice([v for v in range(-amp, amp + 1) if v != 0]))
    h = rng.randint(-2, 3, n).astype(np.float32) + 0.5
    rowptr, col, val = te.csr_of(J)
    rp, ci, vv = [0], [], []
    for i in range(n):
        for k in range(rowptr[i], rowptr[i + 1]):
            if k % 3 == 0:
                ci += [col[k], col[k]]
                vv += [val[k] + 2.0, -2.0]
            else:
                ci.append(col[k])
                vv.append(val[k])
        rp.append(len(ci))
    csr = (np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(vv, np.float32))
    return sf.Built(oracle.Problem(csr=csr, h=h), lambda e: e.set_csr(*csr, h), None, (6.0 * amp, 0.3 * amp))


def _t2():
    import test_baseline_configs_gpu as bc
    from spin_glass_anneal_rl_amd import encoders as enc
    d32, A, B, h, _ = enc.tsp_structure(bc._tsp_distances(6, 106, False), 200.0, 120.0, auto_scale=True)
    csr = oracle.tsp_to_csr(d32, A, B)
    return sf.Built(oracle.Problem(csr=(csr[0].astype(np.int32), csr[1], csr[2]), h=h), lambda e: e.set_tsp(d32, A, B, h),
                    None, (150.0, 3.0))


def _p1():
    import groups_cases as gc
    n, mp, mem, c, h, csr = gc.problem("assignment_5x7")
    return sf.Built(oracle.Problem(csr=csr, h=h), lambda e: e.set_groups(n, (mp, mem), c, h), None, (10.0, 0.1))


def _p2():
    import groups_rest_cases as grc
    n, mp, mem, c, rest, h, csr = grc.problem("colouring_12x3")
    return sf.Built(oracle.Problem(csr=csr, h=h), lambda e: e.set_groups(n, (mp, mem), c, h, rest=rest), None, (10.0, 0.1))


STATIONS = [
    Station("D1", "dense", sf.dense_streaming("i8", True, n=257), leaves="clf_problem, want_i8, table_m"),
    Station("D2", "dense", _d2, leaves="clf_scale = 2 (half-integer h, field cache ON)"),
    Station("D3", "dense", sf.dense_fp64(True), exact=False, leaves="acc64, acc_canon"),
    Station("D4", "dense", sf.dense_fp64(False), leaves="acc64 without acc_canon"),
    Station("D5", "dense", _d5, leaves="from_dense, csr"),
    Station("D6", "dense", _d6, leaves="use_t2, J_bits, row_nnz"),
    Station("B1", "batch", sf.dense_batch(False), leaves="n_models = 3"),
    Station("C1", "csr", sf.csr_forms(4, False, True), leaves="table_scale = 2, rows form"),
    Station("C2", "csr", sf.csr_real(0), exact=False, leaves="canonical csr_acc"),
    Station("C3", "csr", sf.csr_wide(True, packed=True), leaves="slotted, cvp, max_row_len > 256, big_form"),
    Station("C4", "csr", _c4, leaves="csr_sorted = false"),
    Station("G1", "ragged", sf.ragged_batch, leaves="ragged, model_n, d_models"),
    Station("T1", "tsp", sf.tsp(1), leaves="tsp, exact32"),
    Station("T2", "tsp", _t2, exact=False, leaves="tsp without exact32"),
    Station("P1", "groups", _p1, leaves="groups"),
    Station("P2", "groups_rest", _p2, leaves="g_rptr, g_rent"),
]
BY_ID = {s.id: s for s in STATIONS}
BY_KIND = {k: [s.id for s in STATIONS if s.kind == k] for k in KINDS}
assert len(BY_ID) == len(STATIONS) and all(BY_KIND[k] for k in KINDS)
# sga_set_field_cache(ON) is refused while the engine holds a ragged batch (test_ragged_batch_gpu pins that refusal),
# so a station whose settings ask for ON cannot directly follow G1: test_engine_reuse_gpu walks that edge on its own
NEEDS_CACHE_ON = ("D2",)


# ----------------------------------------------------------------------------- walks
def euler_kinds():
    """One Eulerian circuit of the complete digraph on the seven kinds (42 arcs, 43 visits), by a fixed rule: for every
    step d = 1 ... 6 the cycle 0, d, 2d, ... (mod 7), which is closed after seven arcs because 7 is prime; arc (i, j) lies
    on the cycle of d = j - i (mod 7) and on no other."""
    seq = [0]
    for d in range(1, len(KINDS)):
        for _ in range(len(KINDS)):
            seq.append((seq[-1] + d) % len(KINDS))
    return [KINDS[i] for i in seq]


def euler_walks(parts=3):
    """The circuit as station ids, cut into `parts` walks; each starts at the station the one before it ended at.  A
    kind's stations are taken round-robin (one counter per kind over the whole circuit); a station of NEEDS_CACHE_ON
    that would follow a ragged batch gives its turn to the next one of its kind."""
    kinds = euler_kinds()
    turn = {k: 0 for k in KINDS}
    ids = []
    for k in kinds:
        sid = BY_KIND[k][turn[k] % len(BY_KIND[k])]
        turn[k] += 1
        if ids and BY_ID[ids[-1]].kind == "ragged" and sid in NEEDS_CACHE_ON:
            sid = BY_KIND[k][turn[k] % len(BY_KIND[k])]
            turn[k] += 1
        ids.append(sid)
    arcs = len(ids) - 1
    cuts = [round(i * arcs / parts) for i in range(parts + 1)]
    return [ids[cuts[i]:cuts[i + 1] + 1] for i in range(parts)]


EULER = euler_walks()

# value classes inside a kind and across kinds: every flag from set to unset
FIXED = [
    ["D2", "D1", "D3", "D4", "D1", "D6", "D5", "D1"],
    ["C1", "C3", "C2", "C4", "C1"],
    ["C1", "T1"],
    ["C3", "P1"],
    ["D5", "T2", "D1"],
    ["B1", "D1"],
    ["G1", "C1", "G1"],
    ["P2", "P1"],
    ["D3", "P2"],
]


def kind_pairs(walks):
    return {(BY_ID[a].kind, BY_ID[b].kind) for w in walks for a, b in zip(w, w[1:])}


# ----------------------------------------------------------------------------- a visit
def replicas_for(station, R):
    """R rounded up to a whole number of replicas per model (batches split their replicas evenly)."""
    M = len(station.build().models)
    return (R + M - 1) // M * M


def slot_temps(station, R):
    """One ladder per model (a ladder lies within one model), hot to cold."""
    b = station.build()
    M = len(b.models)
    return np.tile(sf.ladder_for(b, R // M), M)


def default_settings(sg):
    """{option: default} as a fresh engine reports them (the environment is read once, in sga_create)."""
    from spin_glass_anneal_rl_amd.engine import option_names
    with sg.AnnealEngine(0) as e:
        return {k: e.get_option(k) for k in option_names()}


_SETTERS = {"set_option": None, "set_tuning": (0, 0), "set_field_cache": ("off",), "set_csr_storage": ("auto",),
            "set_update_rule": (0,)}


def track(e):
    """Note which settings the CALLER touches on engine e (the stations' own set_option / set_tuning / ... calls), so
    that a visit can put exactly those back.  What the library changes on its own -- sga_autotune's pick -- is not the
    caller's: the harness never papers over it."""
    if getattr(e, "_touched", None) is None:
        e._touched, e._plain = set(), {name: getattr(e, name) for name in _SETTERS}
        for name, plain in e._plain.items():
            def call(*a, _name=name, _plain=plain, **kw):
                e._touched.add((_name, a[0]) if _name == "set_option" else (_name,))
                return _plain(*a, **kw)
            setattr(e, name, call)
    return e


def reset_settings(e, defaults):
    """The settings the caller touched back to what a fresh engine has: a walk's stations each bring their own."""
    for item in sorted(track(e)._touched):
        if item[0] == "set_option":
            e._plain["set_option"](item[1], defaults[item[1]])
        else:
            e._plain[item[0]](*_SETTERS[item[0]])
    e._touched.clear()


def refusal(fn, *args):
    """The message of the AnnealingError fn(*args) raises (None: it did not raise)."""
    from spin_glass_anneal_rl_amd.exceptions import AnnealingError
    try:
        fn(*args)
    except AnnealingError as exc:
        return str(exc)
    return None


def collect(e, traces, swapped):
    """Everything a caller can read from an engine that holds a problem and replicas."""
    from spin_glass_anneal_rl_amd import _native as N
    from spin_glass_anneal_rl_amd.engine import option_names
    names = option_names()
    st = {"describe": e.describe(), "explain_route": e.explain_route()}
    q = e.route_query()
    for f, _ in N.RouteQuery._fields_:
        if f == "opt":
            for i in range(N.ROUTE_MAX_OPTS):
                st[f"route_query.opt[{names[i] if i < len(names) else i}]"] = int(q.opt[i])
        else:
            st["route_query." + f] = int(getattr(q, f))
    for m in range(e.n_models if e._sizes is not None else 1):
        try:
            st[f"scan_summary[{m}]"] = e.scan_summary(m)
        except Exception as exc:  # (implicit couplings keep no scan words: the refusal is the answer)
            st[f"scan_summary[{m}]"] = f"{type(exc).__name__}: {exc}"
    st["geometry"] = e.geometry()
    st["last_kernel"] = e.last_kernel()
    st["problem_checksum"] = e.problem_checksum()
    for k in names:
        st["option." + k] = e.get_option(k)
    st["spins"] = e.spins()
    st["spins_of"] = [e.spins(r) for r in range(e.R)]
    st["energies"] = e.energies()
    st["stats.accepted"], st["stats.attempted"] = e.stats()
    best = [e.best(r) for r in range(e.R)]
    st["best.energy"] = np.asarray([b[0] for b in best])
    st["best.spins"] = [b[1] for b in best]
    st["best.replica"] = [b[2] for b in best]
    if e.n_ladders > 0:
        st["slot_map"] = e.slot_map()
        st["exchange_stats.attempts"], st["exchange_stats.accepts"] = e.exchange_stats()
    else:
        st["slot_map"] = refusal(e.slot_map)
        st["exchange_stats.attempts"] = st["exchange_stats.accepts"] = refusal(e.exchange_stats)
    st["counters"] = e.counters()
    st["temperatures"] = e.temperatures()
    st["trace"] = np.vstack(traces)
    st["swapped"] = swapped
    return st


def protocol(e, station, R, seed, ladder, rule=0):
    """init_replicas ... collect on an engine whose problem is set (AnnealEngine, or the oracle's stand-ins)."""
    temps = slot_temps(station, R)
    e.init_replicas(R, seed=seed)
    swapped = None
    if ladder:
        e.set_ladder(temps, len(station.build().models))
    else:
        e.set_temperatures(temps)
    t0 = e.sweep(2, energy_trace=True)["energy_trace"]
    if ladder:
        swapped = e.exchange()
    else:  # free_replicas cleared n_ladders: the last visit's ladder is gone
        msg = refusal(e.exchange)
        assert msg is not None and "no ladder" in msg, (station.id, "exchange() without a ladder", msg)
    t1 = e.sweep(1, energy_trace=True)["energy_trace"]
    return [t0, t1], swapped


def visit(e, station, R, seed, ladder, defaults, pre=None, reset=True):
    """One visit of `station` on engine e.  pre(e): caller settings beyond the station's own, after the reset."""
    R = replicas_for(station, R)
    if reset:
        reset_settings(e, defaults)
    if pre is not None:
        pre(e)
    station.build().setup(e)
    traces, swapped = protocol(e, station, R, seed, ladder)
    return collect(e, traces, swapped)


_FRESH = {}


def fresh(sg, station, R, seed, ladder, defaults, pre=None, key=None):
    """The same visit on a fresh engine, once per (station, R, ladder or not, settings)."""
    k = (station.id, replicas_for(station, R), seed, bool(ladder), key)
    assert pre is None or key is not None, "extra settings need a cache key"
    if k not in _FRESH:
        with track(sg.AnnealEngine(0)) as e:
            _FRESH[k] = visit(e, station, R, seed, ladder, defaults, pre=pre)
    return _FRESH[k]


# ----------------------------------------------------------------------------- comparison
def _same(x, y):
    if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
        return (isinstance(x, np.ndarray) and isinstance(y, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape
                and x.tobytes() == y.tobytes())  # (bytes: an energy that differs in its last bit, or in the sign of zero)
    if isinstance(x, (list, tuple)) and isinstance(y, (list, tuple)):
        return type(x) is type(y) and len(x) == len(y) and all(_same(a, b) for a, b in zip(x, y))
    return type(x) is type(y) and x == y


def assert_same_engine(a, b, tag):
    """a, b: what collect() returned for two engines.  Equal, key by key; the failure names the first differing key
    (a route_query mismatch: "route_query.<field>")."""
    assert list(a) == list(b), (tag, "the two states hold different keys", sorted(set(a) ^ set(b)))
    for key in a:
        if not _same(a[key], b[key]):
            raise AssertionError(f"{tag}: first differing key {key!r}: {a[key]!r} != {b[key]!r}")


# ----------------------------------------------------------------------------- the oracle's side
class _ModelOracle(OracleEngine):
    def __init__(self, prob, rule=0):
        self.prob, self.n, self.R, self.rule = prob, prob.n, 0, rule

    def sweep(self, n_sweeps=1, **kw):
        out = oracle.sweeps(self.prob, self._spins, self._temps, n_sweeps, rule=self.rule, seed=self.seed,
                            sweep0=self.sweeps_done, replica0=self.replica0, energy=self._energy, best_energy=self._best_e)
        better = out["best_energy"] < self._best_e
        self._best_s[better] = out["best_spins"][better]
        self._best_e, self._energy = out["best_energy"], out["energy"]
        self._acc += out["n_accepted"]
        self.sweeps_done += n_sweeps
        return {"energy_trace": out["energy_trace"]}


_ORACLE = {}


def oracle_visit(station, R, seed, ladder, rule=0):
    """The visit's protocol on the CPU oracle, model by model (model m owns global replicas [m k, (m + 1) k) and ladder
    m), in the shape stream_forms.assert_same compares."""
    R = replicas_for(station, R)
    key = (station.id, R, seed, bool(ladder), rule)
    if key in _ORACLE:
        return _ORACLE[key]
    models = station.build().models
    M, k = len(models), R // len(models)
    temps = slot_temps(station, R)
    parts = []
    for m, prob in enumerate(models):
        o = _ModelOracle(prob, rule)
        o.init_replicas(k, seed=seed, R_global=R, replica0=m * k)
        if ladder:
            o.set_ladder(temps, M)
        else:
            o.set_temperatures(temps[m * k:(m + 1) * k])
        t0 = o.sweep(2)["energy_trace"]
        swapped = o.exchange() if ladder else 0
        t1 = o.sweep(1)["energy_trace"]
        parts.append((o, np.vstack([t0, t1]), swapped))
    out = dict(trace=np.hstack([p[1] for p in parts]), spins=[s for p in parts for s in p[0].spins()],
               acc=np.concatenate([p[0].stats()[0] for p in parts]), energy=np.concatenate([p[0].energies() for p in parts]),
               best_e=np.concatenate([p[0]._best_e for p in parts]), best_s=[s for p in parts for s in p[0]._best_s],
               temperatures=np.concatenate([p[0].temperatures() for p in parts]), swapped=sum(p[2] for p in parts),
               counters=(3, 1 if ladder else 0))
    if ladder:
        out["slot_map"] = np.concatenate([p[0].slot_map()[m * k:(m + 1) * k] for m, p in enumerate(parts)])
    _ORACLE[key] = out
    return out


def assert_same_as_oracle(state, station, R, seed, ladder, tag, rule=0):
    """The re-used engine's visit against the CPU oracle: stream_forms.assert_same with the station's own `exact`, then
    what the exchange left (the permutation, the temperatures, the counters)."""
    ref = oracle_visit(station, R, seed, ladder, rule)
    got = dict(trace=state["trace"], spins=state["spins_of"], acc=state["stats.accepted"], energy=state["energies"],
               best_e=state["best.energy"], best_s=state["best.spins"])
    sf.assert_same(got, {k: ref[k] for k in got}, station.exact, (tag, station.id, "against the oracle"))
    assert np.array_equal(state["temperatures"], ref["temperatures"]), (tag, station.id, "temperatures")
    assert tuple(state["counters"]) == ref["counters"], (tag, station.id, "counters")
    if ladder:
        assert state["swapped"] == ref["swapped"], (tag, station.id, "swapped")
        assert np.array_equal(state["slot_map"], ref["slot_map"]), (tag, station.id, "slot_map")


# ----------------------------------------------------------------------------- a walk
def run_walk(sg, e, ids, defaults, tag, start=0, pre=None, key=None, oracle_check=True):
    """Visit the stations `ids` on engine e in order; visit number i (counted from `start`) takes R = R_CYCLE[i % 3] and,
    on every third visit, plain temperatures instead of a ladder.  Every visit equals the fresh engine's; a station's
    last visit in the walk is also held against the oracle.  Returns the last visit's state."""
    last = {sid: i for i, sid in enumerate(ids)}
    state = None
    for i, sid in enumerate(ids):
        st = BY_ID[sid]
        R, ladder = R_CYCLE[(start + i) % len(R_CYCLE)], (start + i) % 3 != 2
        where = f"{tag}: visit {i} ({' -> '.join(ids[max(0, i - 1):i + 1])}), R = {replicas_for(st, R)}, " \
                f"{'ladder' if ladder else 'temperatures'}"
        seed = SEED + STATIONS.index(st)  # (one seed per station: a fresh engine's visit serves every walk)
        state = visit(e, st, R, seed, ladder, defaults, pre=pre)
        assert_same_engine(state, fresh(sg, st, R, seed, ladder, defaults, pre=pre, key=key), where)
        if oracle_check and last[sid] == i:
            assert_same_as_oracle(state, st, R, seed, ladder, where)
    return state
