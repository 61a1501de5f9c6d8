"""Time links and the exchange between Trotter groups along the transverse field (sga_get_time_links,
sga_exchange_transverse, csrc/trotter_exchange.hip), what holds without a GPU: the version, the symbols, the header and the
bindings; the two admission rules run stand-alone (tests/c_abi/trotter_exchange_plan.cpp); the acceptance ratio of the
specification (tests/trotter_exchange_reference.py) against the ratio of the weights exp(-beta H_eff) built from
transverse_reference.effective_energy; the estimators; the configuration; and the specification's own properties
(tests/test_trotter_exchange_gpu.py holds the engine against it)."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import oracle
import transverse_reference as tr
import trotter_exchange_reference as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spin-glass-anneal-rl_amd", "csrc")
SEED = (33 << 32) | 3300


@pytest.fixture(scope="module")
def sg():
    import spin_glass_anneal_rl_amd as m
    return m


def test_version_symbols_header_bindings(sg):
    lib = sg._native.lib()
    assert lib.sga_version() >= 3300
    assert hasattr(lib, "sga_get_time_links") and hasattr(lib, "sga_exchange_transverse")
    sym = {s[0]: s for s in sg._native.SYMBOLS}
    assert len(sym["sga_get_time_links"][2]) == 3 and len(sym["sga_exchange_transverse"][2]) == 7
    header = open(os.path.join(ROOT, "include", "sga.h")).read()
    assert "int sga_get_time_links(sga_engine *e, int n_slices, int64_t *links" in header
    assert "int sga_exchange_transverse(sga_engine *e, int n_slices, const float *k_perp" in header
    text = header[header.index("time links and the exchange along the transverse field (version >= 3300"):header.index("int sga_get_time_links(")]
    for phrase in ("t2  = (2.0 * c) * (double)(B_a - B_b)", "counter (0, round, a, 8)", "STAY VALID", "parity must be 0 or 1",
                   "links is NULL", "R_local == R_global"):
        assert phrase in text, phrase
    dev = open(os.path.join(CSRC, "sga_device.h")).read()
    assert "DOMAIN_TROTTER_EXCHANGE = DOMAIN_SWEEP | (2u << 2)" in dev and xr.DOMAIN_TROTTER_EXCHANGE == 8
    assert "philox4x32_10(" not in open(os.path.join(CSRC, "trotter_exchange.hip")).read()  # the draw is sweep_common.h's
    assert "trotter_exchange_u(" in open(os.path.join(CSRC, "sweep_common.h")).read()
    a = inspect.signature(sg.AnnealEngine.time_links).parameters
    assert list(a) == ["self", "n_slices", "out"] and a["out"].default is None
    b = inspect.signature(sg.AnnealEngine.exchange_transverse).parameters
    assert list(b) == ["self", "n_slices", "k_perp", "parity", "round"] and b["parity"].default is None and b["round"].default is None
    for name in ("transverse_magnetization", "quantum_energy"):
        assert name in sg.__all__ and getattr(sg, name) is getattr(sg.quantum, name)


# ---- the admission rules, stand-alone ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("trotter_exchange_plan")), "trotter_exchange_plan")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-I", "/opt/rocm/include",
                    os.path.join(ROOT, "tests", "c_abi", "trotter_exchange_plan.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


SERVED = dict(have_engine=1, have_array=1, n=100, R_local=12, replica0=0, csr=0, tsp=0, groups=0, ragged=0, n_models=1,
              clf_problem=1, metropolis=1, n_slices=4)


def links(exe, **change):
    q = dict(SERVED, **change)
    return subprocess.run([exe, "links"] + [str(q[key]) for key in SERVED], check=True, capture_output=True, text=True).stdout.strip()


def exchange(exe, k=(0.5,), parity=0, R_global=None, **change):
    q = dict(SERVED, **change)
    rg = q["R_local"] if R_global is None else R_global
    out = subprocess.run([exe, "exchange"] + [str(q[key]) for key in SERVED] + [str(rg), str(parity)] + [str(x) for x in k],
                         check=True, capture_output=True, text=True)
    return out.stdout.strip()


LADDER = {"engine is NULL": dict(have_engine=0), "no couplings set": dict(n=0),
          "no replicas (call sga_init_replicas)": dict(R_local=0), "n_slices must be at least 2": dict(n_slices=1),
          "n_slices must divide the number of local replicas": dict(n_slices=5),
          "replica0 must be a multiple of n_slices (groups lie whole on a rank)": dict(replica0=6)}
KINDS = {"sga_set_tsp": dict(tsp=1), "sga_set_groups": dict(groups=1), "ragged": dict(ragged=1, csr=1, n_models=3),
         "batches": dict(n_models=3)}


def test_time_links_admission(plan_exe):
    assert links(plan_exe) == "ok"
    for P in (2, 3, 4, 6, 12):  # odd P included
        assert links(plan_exe, n_slices=P) == "ok", P
    assert links(plan_exe, n_slices=66, R_local=132) == "ok"  # no upper bound
    assert links(plan_exe, replica0=8) == "ok" and links(plan_exe, R_local=4, replica0=4) == "ok"
    # no coupling is read: CSR of any class, a dense problem outside the integer form, any rule
    assert links(plan_exe, csr=1) == "ok" and links(plan_exe, clf_problem=0) == "ok" and links(plan_exe, metropolis=0) == "ok"
    for word, change in dict(LADDER, **{"links is NULL": dict(have_array=0)}).items():
        assert links(plan_exe, **change) == "invalid: " + word, change
    assert links(plan_exe, have_engine=0, have_array=0) == "invalid: engine is NULL"  # the ladder's order
    assert links(plan_exe, have_array=0, n=0) == "invalid: links is NULL"
    for P in (0, -2, 8, 24):
        assert links(plan_exe, n_slices=P).startswith("invalid: n_slices"), P
    for word, change in KINDS.items():
        out = links(plan_exe, **change)
        assert out.startswith("unsupported: time links are not implemented for ") and word in out, (change, out)
        assert links(plan_exe, n_slices=5, **change).startswith("invalid: "), change  # an argument error wins over the kind


def test_exchange_admission(plan_exe):
    assert exchange(plan_exe) == "ok" and exchange(plan_exe, parity=1) == "ok"
    for P in (2, 3, 4, 6, 12):
        assert exchange(plan_exe, n_slices=P) == "ok", P
    assert exchange(plan_exe, n_slices=66, R_local=132) == "ok"
    assert exchange(plan_exe, csr=1) == "ok" and exchange(plan_exe, clf_problem=0) == "ok" and exchange(plan_exe, metropolis=0) == "ok"
    assert exchange(plan_exe, k=(0.0, -1.0, 5.0)) == "ok"
    for word, change in dict(LADDER, **{"k_perp is NULL": dict(have_array=0)}).items():
        assert exchange(plan_exe, **change) == "invalid: " + word, change
    for k in (("nan",), ("inf",), (0.5, 0.5, "nan")):  # (the third and last of the G = 3 values)
        assert exchange(plan_exe, k=k) == "invalid: k_perp holds a NaN or an infinite value", k
    assert exchange(plan_exe, k=(0.5, 0.5, 0.5, "nan")) == "ok"  # only the G values are read
    # the two new texts, in their order behind the ladder
    for parity in (2, -1):
        assert exchange(plan_exe, parity=parity) == "invalid: parity must be 0 or 1"
    assert exchange(plan_exe, R_global=24) == "invalid: exchanges between groups need every group on this rank (R_local == R_global)"
    assert exchange(plan_exe, parity=2, R_global=24) == "invalid: parity must be 0 or 1"
    assert exchange(plan_exe, parity=2, k=("nan",)) == "invalid: k_perp holds a NaN or an infinite value"
    assert exchange(plan_exe, parity=2, n_slices=5) == "invalid: n_slices must divide the number of local replicas"
    for word, change in KINDS.items():
        out = exchange(plan_exe, **change)
        assert out.startswith("unsupported: transverse-field exchanges are not implemented for ") and word in out, (change, out)
        for wrong in (dict(n_slices=5), dict(parity=2), dict(R_global=24), dict(k=("nan",))):  # invalid before unsupported
            assert exchange(plan_exe, **dict(change, **wrong)).startswith("invalid: "), (change, wrong)


# ---- the ratio is the ratio of the weights ------------------------------------------------------------------------------------------
def small_problem(n, rng):
    J = np.triu(rng.randint(-3, 4, (n, n)), 1).astype(np.float32)
    return oracle.Problem(J=J + J.T, h=(rng.randint(-2, 3, n) / 2.0).astype(np.float32))


@pytest.mark.parametrize("P", [2, 4])
def test_x_is_the_log_ratio_of_the_weights(P):
    """log[w(S_b; a) w(S_a; b) / (w(S_a; a) w(S_b; b))] with w(S; g) = exp(-H_eff(S, k_g) / T_g), H_eff from
    transverse_reference.effective_energy, against x of decide.  The four log weights cancel against each other, so the
    tolerance 1e-12 is relative to the largest of them: it checks the derivation, not bits."""
    rng = np.random.RandomState(100 + P)
    checked = 0
    for trial in range(40):
        n = int(rng.randint(2, 9))
        prob = small_problem(n, rng)
        S = (rng.randint(0, 2, (2 * P, n)) * 2 - 1).astype(np.int8)
        if trial % 4 == 0:
            S[P + 1:] = S[P]  # a group with few broken links
        T = np.repeat(rng.uniform(0.5, 4.0, 2), P)
        k = rng.uniform(0.05, 3.0, 2).astype(np.float32)
        E = np.asarray([oracle.energy(prob, s) for s in S])
        B = xr.time_links(S, P)
        assert np.all(B % 2 == 0) and np.all(B <= n * P)
        (d,) = xr.decide(E, T, k, B, P, 0, SEED, trial)
        Sa, Sb = S[:P], S[P:]
        logw = lambda s, g: -tr.effective_energy(prob, s, P, float(k[g])) / T[g * P]  # noqa: E731
        terms = [logw(Sb, 0), logw(Sa, 1), -logw(Sa, 0), -logw(Sb, 1)]
        want = sum(terms)
        assert abs(d["x"] - want) <= 1e-12 * max(abs(t) for t in terms), (trial, d["x"], want)
        assert d["prob"] == (1.0 if not d["x"] < 0.0 else oracle.exp(d["x"])) and d["swap"] == (d["u"] < d["prob"])
        checked += d["x"] != 0.0
    assert checked >= 30


# ---- the estimators --------------------------------------------------------------------------------------------------------------------
def test_estimators(sg):
    m, q = sg.transverse_magnetization, sg.quantum_energy
    n, P, gamma, T = 10, 4, 1.5, 0.25
    a = gamma / (P * T)
    assert m(0, n, P, gamma, T) == np.tanh(a) and m(n * P, n, P, gamma, T) == 1.0 / np.tanh(a)
    assert isinstance(m(0, n, P, gamma, T), float)
    half = m(n * P // 2, n, P, gamma, T)
    assert abs(half - 0.5 * (np.tanh(a) + 1.0 / np.tanh(a))) < 1e-15
    # arrays broadcast: links [G] against gamma [G], and against a scalar
    B = np.asarray([0, 8, 40], np.int64)
    g = np.asarray([0.5, 1.0, 2.0])
    out = m(B, n, P, g, T)
    assert out.shape == (3,) and out.dtype == np.float64
    assert np.array_equal(out, [m(int(B[i]), n, P, float(g[i]), T) for i in range(3)])
    assert m(B[:, None], n, P, g[None, :], T).shape == (3, 3)
    E = np.arange(12, dtype=np.float64).reshape(3, 4)
    qe = q(E, B, n, P, g, T)
    assert qe.shape == (3,) and np.array_equal(qe, E.mean(axis=1) - g * n * out)
    assert isinstance(q(E[0], 0, n, P, gamma, T), float) and q(E[0], 0, n, P, gamma, T) == 1.5 - gamma * n * np.tanh(a)


# ---- the configuration -----------------------------------------------------------------------------------------------------------------
def test_config(sg):
    C = sg.SimulatedQuantumAnnealingConfig
    assert C().field_ladder is None and C().field_exchange_interval == 0
    ok = C(n_instances=3, field_ladder=[0.5, 1.0, 2.0], field_exchange_interval=2)
    assert ok.field_exchange_interval == 2
    with pytest.raises(sg.ConfigurationError, match="one multiplier per instance"):
        C(n_instances=3, field_ladder=[1.0, 2.0])
    with pytest.raises(sg.ConfigurationError, match="one multiplier per instance"):
        C(n_instances=1, field_ladder=[[1.0]])
    for bad in ([1.0, 0.0, 2.0], [1.0, -1.0, 2.0], [1.0, np.nan, 2.0], [1.0, np.inf, 2.0]):
        with pytest.raises(sg.ConfigurationError, match="positive finite multipliers"):
            C(n_instances=3, field_ladder=bad)
    with pytest.raises(sg.ConfigurationError, match="n_instances >= 2"):
        C(field_exchange_interval=1)
    for bad in (-1, 1.5, True, None):
        with pytest.raises(sg.ConfigurationError, match="field_exchange_interval must be a non-negative integer"):
            C(n_instances=2, field_exchange_interval=bad)
    assert C(n_instances=2, field_exchange_interval=3).field_ladder is None  # an exchange without a ladder is allowed
    # couplings_by_instance: [n_sweeps, G]; multipliers all 1 give couplings() in every column
    c = C(n_instances=3, n_sweeps=7, n_slices=4)
    kb = c.couplings_by_instance()
    assert kb.shape == (7, 3) and kb.dtype == np.float32
    ones = C(n_instances=3, n_sweeps=7, n_slices=4, field_ladder=[1.0, 1.0, 1.0])
    for col in range(3):
        assert np.array_equal(kb[:, col], c.couplings()) and np.array_equal(ones.couplings_by_instance()[:, col], c.couplings())
    lad = C(n_instances=3, n_sweeps=7, n_slices=4, field_ladder=[0.5, 1.0, 2.0])
    assert np.array_equal(lad.couplings(), c.couplings())  # couplings() keeps its meaning
    kl = lad.couplings_by_instance()
    assert np.array_equal(kl[:, 1], c.couplings()) and np.all(kl[:, 0] > kl[:, 1]) and np.all(kl[:, 1] > kl[:, 2])
    want = sg.transverse_coupling(0.5 * c.transverse_field.gammas(7), c.temperature, 4).astype(np.float32)
    assert np.array_equal(kl[:, 0], want)
    q = sg.QuantumFluctuations(None, "constant", 2.0, n_instances=2, field_ladder=[1.0, 2.0], field_exchange_interval=4)
    assert q.field_ladder == (1.0, 2.0) and q.field_exchange_interval == 4
    q = sg.QuantumFluctuations(None, "constant", 2.0)
    assert q.field_ladder is None and q.field_exchange_interval == 0
    with pytest.raises(sg.ConfigurationError, match="n_instances >= 2"):
        sg.QuantumFluctuations(None, "constant", 2.0, field_exchange_interval=2).path_integral_mc(None, 4)


# ---- the specification's own properties ---------------------------------------------------------------------------------------------------
def random_state(G, P, n, rng):
    S = (rng.randint(0, 2, (G * P, n)) * 2 - 1).astype(np.int8)
    E = rng.randint(-20, 21, G * P).astype(np.float64)
    return S, E


def test_u53_and_draw():
    assert xr.u53(0, 0) == 0.0 and xr.u53(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53
    assert xr.u53(1 << 5, 0) == 2.0 ** -27 and xr.u53(0, 1 << 6) == 2.0 ** -53
    base = xr.draw(SEED, 3, 2)
    assert len({base, xr.draw(SEED, 4, 2), xr.draw(SEED, 3, 1), xr.draw(SEED ^ 1, 3, 2), xr.draw(SEED ^ (1 << 32), 3, 2)}) == 5
    assert xr.draw(SEED, 2 ** 32 + 3, 2) == base and 0.0 <= base < 1.0
    w = oracle.philox((0, 3, 2, 8), (SEED & 0xFFFFFFFF, SEED >> 32))
    assert base == xr.u53(w[0], w[1])


@pytest.mark.parametrize("G", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("parity", [0, 1])
def test_equal_parameters_swap_every_pair(G, parity):
    P, n = 4, 9
    rng = np.random.RandomState(G * 2 + parity)
    S, E = random_state(G, P, n, rng)
    T, k = np.full(G * P, 3.0), np.full(G, 0.75, np.float32)
    out = xr.apply(S, E, E + 100.0, S, T, k, P, parity, SEED, 5)
    assert all(d["x"] == 0.0 and d["prob"] == 1.0 and d["swap"] for d in out["decisions"])
    assert [(d["a"], d["b"]) for d in out["decisions"]] == [(a, a + 1) for a in range(parity, G - 1, 2)]
    want = np.zeros(G, np.int32)
    for d in out["decisions"]:
        want[[d["a"], d["b"]]] = 1
    assert np.array_equal(out["accepted"], want)
    # a permutation of the rows: every row of the state is where the pairs put it, with its energy
    perm = np.arange(G * P)
    for d in out["decisions"]:
        a, b = d["a"], d["b"]
        perm[a * P:(a + 1) * P], perm[b * P:(b + 1) * P] = np.arange(b * P, (b + 1) * P), np.arange(a * P, (a + 1) * P)
    assert sorted(perm) == list(range(G * P))
    assert np.array_equal(out["spins"], S[perm]) and np.array_equal(out["energy"], E[perm])
    assert np.array_equal(out["links"], xr.time_links(S, P)) and np.all(out["links"] % 2 == 0)
    assert np.array_equal(xr.time_links(out["spins"], P), out["links"][perm[::P] // P])
    # the bests follow the rows that are lower now
    assert np.array_equal(out["best_energy"], np.minimum(E + 100.0, out["energy"])) and np.array_equal(out["best_spins"], out["spins"])


def test_time_links_of_made_states():
    n = 7
    s = (np.arange(n) % 2 * 2 - 1).astype(np.int8)
    for P in (2, 3, 4, 5):
        same = np.repeat(s[None, :], P, axis=0)
        assert xr.time_links(same, P)[0] == 0
        one = same.copy()
        one[P - 1, 3] *= -1
        assert xr.time_links(one, P)[0] == 2  # P = 2: the one differing site counts for both links
        if P % 2 == 0:
            alt = np.stack([s if p % 2 == 0 else -s for p in range(P)])
            assert xr.time_links(alt, P)[0] == n * P
    rng = np.random.RandomState(1)
    for P in (2, 3, 6):
        B = xr.time_links((rng.randint(0, 2, (3 * P, n)) * 2 - 1).astype(np.int8), P)
        assert B.shape == (3,) and B.dtype == np.int64 and np.all(B % 2 == 0) and np.all(B <= n * P)


def test_unusable_temperatures_leave_their_pairs_alone():
    P, n, G = 2, 5, 4
    S, E = random_state(G, P, n, np.random.RandomState(9))
    k = np.full(G, 0.5, np.float32)
    for bad in (0.0, np.inf, -1.0, np.nan):
        T = np.repeat([2.0, bad, 2.0, 2.0], P)
        out = xr.apply(S, E, E, S, T, k, P, 0, SEED, 1)
        assert [d["swap"] for d in out["decisions"]] == [False, True] and out["decisions"][0]["x"] is None
        assert np.array_equal(out["accepted"], [0, 0, 1, 1])
        assert np.array_equal(out["spins"][:2 * P], S[:2 * P]) and np.array_equal(out["spins"][2 * P:3 * P], S[3 * P:])
