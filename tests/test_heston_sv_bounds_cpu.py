"""What the Heston price bounds with a policy on the spot and the variance state (omc_price_american_bounds_heston with
cfg.regressors = 1) offer without a GPU: the selector's field and the unchanged symbol set and ABI
version, the facade's and the context method's argument checks, and the numpy restatement's own pieces
(tests/helpers/heston_sv_ref.py) -- the stop rule on hand-written rows, the fit through runnerup_ref.ldl_fit against
numpy.linalg.lstsq with its truncation cases, and the fuzz cases, every one restated on float32 numpy paths without a tie
(the convention of test_fuzz_cases_cpu.py)."""
import hashlib

import numpy as np
import pytest

from helpers import heston_bounds_case as hc
from helpers import heston_sv_ref as sv
from helpers import runnerup_ref as rr
from options_model_amd import _ffi
from oracle import cpu as orc

K = 100.0
FELLER_OFF = dict(v0=0.04, kappa=1.0, theta=0.09, xi=0.9, rho=-0.7)


# ------------------------------------------------------------------ the interface
def test_selector_field_symbols_and_abi_version():
    assert _ffi.BoundsConfig.regressors.offset == 4 and _ffi.BoundsConfig.regressors.size == 4
    assert [n for n, _ in _ffi.BoundsConfig._fields_][:3] == ["policy", "regressors", "n_lower"]
    assert not hasattr(_ffi.BoundsConfig, "reserved")
    assert _ffi.BoundsConfig().regressors == 0  # a fresh config asks for the spot-only policy
    assert _ffi.HESTON_BOUND_REGRESSORS == ("spot", "spot+variance")
    lib = _ffi.load_library()
    assert lib.omc_abi_version() == 14 == _ffi.ABI_VERSION
    assert len(lib.omc_price_american_bounds_heston.argtypes) == 8


def test_no_new_exported_symbol():
    """the selector travels in omc_bounds_config: the set of entry points is what it was before this policy family (80 names,
    fingerprinted), so tests/test_call_catalogue_cpu.py needs no new call"""
    names = sorted(_ffi.SIGNATURES)
    assert len(names) == 80
    assert hashlib.sha256("\n".join(names).encode()).hexdigest() == \
        "f02ca079bac6a6a0ba8fbf0ee004c5cd8587c4cc7283c852c525b89f1749c9d9"
    assert [n for n in names if "heston" in n and "bounds" in n] == ["omc_price_american_bounds_heston"]
    assert not [n for n in names if "_sv_bounds" in n or "heston_sv" in n or "variance" in n]
    lib = _ffi.load_library()
    for n in ("omc_price_american_bounds_heston_sv", "omc_price_american_heston_sv_bounds"):
        assert not hasattr(lib, n)


@pytest.mark.parametrize("kw,match", [
    (dict(regressors="spot+vol"), "regressors"), (dict(regressors="index"), "regressors"),
    (dict(policy="two_pass"), "textbook"), (dict(policy="reference"), "textbook"),
    (dict(policy="given", betas=np.zeros((5, 4))), r"\(5, 8\)"), (dict(policy="given", betas=np.zeros((6, 8))), r"\(5, 8\)"),
    (dict(n_steps=513), "512"),
    (dict(heston_params=dict(v0=0.0, kappa=2.0, theta=0.0, xi=0.3, rho=-0.7)), r"max\(v0, theta\)"),
    (dict(heston_params=dict(v0=0.0, kappa=2.0, theta=-0.01, xi=0.3, rho=-0.7)), r"max\(v0, theta\)")],
    ids=["unknown", "basket-value", "two_pass", "reference", "betas-cols", "betas-rows", "513-steps", "vbar-zero",
         "vbar-negative"])
def test_facade_refuses_before_the_device(kw, match):
    """no context is given and none is made (device 10^6 does not exist): the checks come first.  On the code before this
    policy family the keyword itself is a TypeError."""
    from options_model_amd import price_american_bounds_heston

    args = dict(S0=100.0, K=K, r=0.05, T=1.0, n_paths=1000, n_steps=4, heston_params=hc.HP, device=10 ** 6,
                regressors="spot+variance")
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        price_american_bounds_heston(**args)


def test_facade_default_is_the_spot_policy():
    """regressors="spot" keeps every check of the spot-only call: a [N+1][8] table is refused there, 513 steps are not"""
    from options_model_amd import HestonBoundsResult, BoundsResult, price_american_bounds_heston

    assert issubclass(HestonBoundsResult, BoundsResult)
    assert [f for f in HestonBoundsResult.__dataclass_fields__ if f not in BoundsResult.__dataclass_fields__] == \
        ["regressors", "variance_scale"]
    args = dict(S0=100.0, K=K, r=0.05, T=1.0, n_paths=1000, n_steps=4, heston_params=hc.HP, device=10 ** 6)
    with pytest.raises(ValueError, match=r"\(5, 4\)"):
        price_american_bounds_heston(policy="given", betas=np.zeros((5, 8)), **args)
    with pytest.raises(ValueError, match=r"\(5, 4\)"):
        price_american_bounds_heston(policy="given", betas=np.zeros((5, 8)), regressors="spot", **args)


def test_context_method_checks_regressors_and_betas_shape():
    ctx = object.__new__(_ffi.Context)  # never opened: the checks need no device
    ctx.handle = None
    p = hc.make_params(hc.HP, N=5)
    with pytest.raises(ValueError, match=r"\(6, 8\)"):
        ctx.price_american_bounds_heston(p, policy="given", betas=np.zeros((6, 4)), regressors="spot+variance")
    with pytest.raises(ValueError, match=r"\(6, 8\)"):
        ctx.price_american_bounds_heston(p, policy="given", betas=np.zeros((6, 4)), regressors=1)
    with pytest.raises(ValueError, match=r"\(6, 4\)"):
        ctx.price_american_bounds_heston(p, policy="given", betas=np.zeros((6, 8)))
    with pytest.raises(ValueError, match="regressors"):
        ctx.price_american_bounds_heston(p, regressors="variance")


# ------------------------------------------------------------------ the helper's rule
def test_stop_rule_on_hand_written_rows():
    N, t, vbar = 4, 2, 0.05
    b = np.zeros((N + 1, 8))
    b[t] = (5.0, 0.0, 0.0, 10.0, 0.0, 0.0, 7.0, 0.0)  # cont = 5 + 10 w, w = V / 0.05 - 1
    X = np.array([90.0, 90.0, 94.0, 101.0, 90.0], np.float32)
    Y = np.array([0.05, 0.09, 0.0625, 0.2, -0.0125], np.float32)  # w = 0, 0.8, 0.25, ., -1.25 -> cont = 5, 13, 7.5, ., -7.5
    st, ties = sv.stop_rule(X, Y, t, N, K, True, b, vbar)
    np.testing.assert_array_equal(st, [True, False, False, False, True])  # imm = 10, 10, 6, out of the money, 10
    assert ties == 0
    st, ties = sv.stop_rule(X, Y, t, N, K, True, b, 2 * vbar)  # the scale is part of the rule: w = -0.5, -0.1, ...
    np.testing.assert_array_equal(st[:3], [True, True, True])
    # a negative variance state of scheme 1 is a regressor like any other; a tie is a decision within TIE * K
    b[t][0] = 10.0
    Y0 = np.array([0.0625], np.float32)  # exact in float32: w = 0 at vbar = 0.0625, cont = 10 = imm
    st, ties = sv.stop_rule(X[:1], Y0, t, N, K, True, b, 0.0625)
    assert ties == 1 and not st[0]
    b[t][0] = 10.0 - 5e-6
    st, ties = sv.stop_rule(X[:1], Y0, t, N, K, True, b, 0.0625)
    assert ties == 0 and st[0]
    b[t][6] = 0.0
    assert not sv.stop_rule(X, Y, t, N, K, True, b, vbar)[0].any()  # nobody was in the money there: no exercise
    assert sv.stop_rule(X, Y, N, N, K, True, b, vbar)[0].all()
    # with c3 = c4 = c5 = 0 the variance does not enter
    b[t] = (5.0, -30.0, 2.0, 0.0, 0.0, 0.0, 7.0, 0.0)
    a, _ = sv.stop_rule(X, Y, t, N, K, True, b, vbar)
    c, _ = sv.stop_rule(X, Y[::-1].copy(), t, N, K, True, b, vbar)
    np.testing.assert_array_equal(a, c)


def test_first_stop_takes_the_first_date_and_its_spot():
    N, vbar = 3, 0.04
    b = np.zeros((N + 1, 8))
    b[1] = b[2] = (0.0, 0.0, 0.0, 100.0, 0.0, 0.0, 5.0, 0.0)  # cont = 100 w: exercise in the money when V < vbar
    X = np.array([[100, 100, 100], [95, 95, 105], [90, 97, 90], [80, 99, 120]], np.float32)
    Y = np.array([[.04, .04, .04], [.05, .03, .03], [.03, .03, .03], [.04, .04, .04]], np.float32)
    tau, x, Z, ties = sv.first_stop(X, Y, 0, N, K, 0.0, 1.0, True, b, vbar)
    np.testing.assert_array_equal(tau, [2, 1, 2])
    np.testing.assert_array_equal(x, [90.0, 95.0, 90.0])
    np.testing.assert_array_equal(Z, [10.0, 5.0, 10.0])
    assert ties == 0
    tau, x, _, _ = sv.first_stop(X[1:], Y[1:], 1, N, K, 0.0, 1.0, True, b, vbar)  # started at date 1: date 1 is not a stop
    np.testing.assert_array_equal(tau, [2, 2, 2])


def test_table_conversions():
    b4 = np.array([[0, 0, 0, 0], [1.0, 2.0, 3.0, 9.0], [0, 0, 0, 0]])
    b8 = sv.lifted_table(b4)
    assert b8.shape == (3, 8) and list(b8[1]) == [1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 9.0, 0.0]
    np.testing.assert_array_equal(sv.spot_table(b8), b4)
    b8[1][4] = 1.0
    with pytest.raises(AssertionError):
        sv.spot_table(b8)


# ------------------------------------------------------------------ the helper's fit
def _regression_set(rng, n, vbar=0.09):
    X = (100.0 * np.exp(rng.normal(-0.1, 0.2, n))).astype(np.float32)
    Y = (vbar * rng.gamma(2.0, 0.4, n) - 0.01).astype(np.float32)  # some negative states
    u, w = sv.uw(X, Y, K, vbar)
    y = np.maximum(6.0 - 40.0 * u + 9.0 * w - 15.0 * u * w + rng.normal(0.0, 5.0, n), 0.0)
    return u, w, y


@pytest.mark.parametrize("n", [20, 300, 5000, 100_000])
def test_fit_equals_lstsq(n):
    """fitted values on the set within 1e-9 K (check_fit's tolerance) of numpy's SVD solve"""
    worst = 0.0
    for s in range(10 if n < 100_000 else 3):
        u, w, y = _regression_set(np.random.default_rng(1000 * n + s), n)
        assert w.min() < -1.0 or n < 300  # negative variance states are in the set
        row = rr.ldl_fit(u, w, y)
        G = np.stack([np.ones(n), u, u * u, w, w * w, u * w], axis=1)
        coef = np.linalg.lstsq(G, y, rcond=None)[0]
        assert row[6] == n and row[7] == 0.0
        diff = float(np.max(np.abs(G @ coef - rr.continuation(u, w, row))))
        worst = max(worst, diff)
        assert diff <= 1e-9 * K, (n, s, diff)
    print(f"n = {n}: largest difference of fitted values {worst:.3g}")


def test_fit_truncation_cases():
    """w exactly 0 on every path (xi = 0, v0 = theta exact in float32): the centred w column is zero, so w and every later
    feature get coefficient 0 exactly and what is left is the quadratic in u; fewer rows than coefficients; an empty set"""
    rng = np.random.default_rng(7)
    u, _, y = _regression_set(rng, 500)
    X = (K * (u + 1.0)).astype(np.float32)
    u2, w = sv.uw(X, np.full(500, 0.0625, np.float32), K, 0.0625)
    assert not w.any()
    row = rr.ldl_fit(u2, w, y)
    assert not row[3:6].any() and row[6] == 500
    coef = np.linalg.lstsq(np.stack([np.ones(500), u2, u2 * u2], axis=1), y, rcond=None)[0]
    np.testing.assert_allclose(row[:3], coef, rtol=1e-9, atol=1e-9)
    r2 = rr.ldl_fit(np.array([0.1, 0.2]), np.array([0.0, 0.05]), np.array([3.0, 5.0]))
    assert r2[6] == 2 and not r2[2:6].any() and np.allclose(r2[:2], (1.0, 20.0))
    r1 = rr.ldl_fit(np.array([0.1]), np.array([0.0]), np.array([3.0]))
    assert r1[0] == 3.0 and not r1[1:6].any() and r1[6] == 1
    assert not rr.ldl_fit(np.zeros(0), np.zeros(0), np.zeros(0)).any()


def test_fit_table_and_check_fit_agree():
    """fit_table's rows pass check_fit on the paths they were fitted on, and a changed row does not"""
    N, M = 6, 2000
    z = orc.gbm_normals(M // 2, 2 * N, 11, 0, 0)
    X, Y = sv.paths_f32(z[0::2], z[1::2], 100.0, 0.04, 0.05, 1.0, 1.0, 0.09, 0.9, -0.7, 1)
    assert Y.min() < 0.0  # Feller violated, scheme 1: negative states are in the regression
    b, ties = sv.fit_table(X, Y, K, 0.05, 1.0, True, 0.09)
    assert ties == 0 and b[1:N, 6].min() > 100 and b[1:N, 3:6].any()
    assert sv.check_fit(X, Y, K, 0.05, 1.0, True, b, 0.09) <= 1e-12
    bad = b.copy()
    bad[3][3] += 1e-3
    with pytest.raises(AssertionError):
        sv.check_fit(X, Y, K, 0.05, 1.0, True, bad, 0.09)


# ------------------------------------------------------------------ float32 Heston in numpy
def test_paths_f32_floor_and_partners():
    N, H = 13, 500
    z = orc.gbm_normals(H, 2 * N, 5, 2, 0)
    for scheme in (0, 1):
        S, V = sv.paths_f32(z[0::2], z[1::2], 100.0, 0.04, 0.05, 1.0, 1.0, 0.09, 0.9, -0.7, scheme)
        assert S.shape == V.shape == (N + 1, 2 * H) and S.dtype == V.dtype == np.float32
        assert np.all(S > 0) and np.all(np.isfinite(V)) and np.all(V[0] == np.float32(0.04))
        assert (V.min() >= 0.0 and (V == 0).any()) if scheme == 0 else V.min() < 0.0
        assert np.any(V[1:, :H] != V[1:, H:])
    # xi = 0 and v0 = theta: the variance never moves
    S, V = sv.paths_f32(z[0::2], z[1::2], 100.0, 0.0625, 0.05, 1.0, 2.0, 0.0625, 0.0, -0.7, 0)
    assert np.all(V == np.float32(0.0625))


# ------------------------------------------------------------------ the fuzz cases
CASES = sv.fuzz_cases(8)


def test_fuzz_cases_cover_what_they_promise():
    assert CASES == sv.fuzz_cases(8) and CASES == sv.fuzz_cases(12)[:8]  # seeded: the same cases every time
    assert all(1 <= c["N"] <= 13 and c["n_inner"] in hc.N_INNER for c in CASES)
    assert {c["n_inner"] for c in CASES} == {2, 64, 130, 200} and len({c["n_outer"] for c in CASES}) > 3
    assert all(c["n_outer"] % 2 == 0 and 2 <= c["n_outer"] <= 40 for c in CASES)
    assert {c["scheme"] for c in CASES} == {0, 1} and {c["is_put"] for c in CASES} == {True, False}
    assert [c["policy"] for c in CASES] == ["textbook", "given"] * 4
    assert any(any(c["holes"][1:c["N"]]) for c in CASES if c["policy"] == "given")
    off = [k for k, c in enumerate(CASES) if not c["feller"]]
    assert off == [2, 5] and {CASES[k]["policy"] for k in off} == {"textbook", "given"}
    assert all("irr_every" not in c and max(c["v0"], c["theta"]) > 0 for c in CASES)


def _numpy_states(c, n_paths, stream, off=0, s0=None, v0=None):
    z = orc.gbm_normals(n_paths // 2, 2 * c["N"], c["seed"], stream, off)
    return sv.paths_f32(z[0::2], z[1::2], c["S0"] if s0 is None else s0, c["v0"] if v0 is None else v0, c["r"], c["T"],
                        c["kappa"], c["theta"], c["xi"], c["rho"], c["scheme"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"N{c['N']}-i{c['n_inner']}-s{c['scheme']}-{c['policy']}")
def test_fuzz_case_restates_without_ties(case):
    """every case through the restatement on float32 numpy paths at the case's Philox coordinates: no decision within
    1e-10 K of the continuation value, in the fit, the lower sweep, the inner simulations or the walk"""
    c = case
    N, vbar, H = c["N"], max(c["v0"], c["theta"]), c["n_inner"] // 2
    kw = (c["K"], c["r"], c["T"], c["is_put"])
    if c["policy"] == "given":
        b, ties = sv.fit_table(*_numpy_states(c, 2048, 9), *kw, vbar)
        b[np.asarray(c["holes"]), 6] = 0.0
    else:
        b, ties = sv.fit_table(*_numpy_states(c, c["M"], c["stream"]), *kw, vbar)
    assert ties == 0
    Xo, Yo = _numpy_states(c, c["n_outer"], c["stream"] + 2)

    def inner(i, t):
        X, Y = _numpy_states(c, c["n_inner"], c["stream"] + 3, (i * (N + 1) + t) * H, float(Xo[t, i]), float(Yo[t, i]))
        return X[:N - t + 1], Y[:N - t + 1]

    lo = sv.lower_bound(*_numpy_states(c, c["n_lower"], c["stream"] + 1), *kw, b, vbar)
    up = sv.upper_bound(Xo, Yo, inner, *kw, b, vbar)
    assert lo["ties"] == 0 and up["ties"] == 0
    assert up["q"].shape == (c["n_outer"], N) and np.all(up["q"] >= 0.0)
    assert c["n_outer"] * c["n_inner"] * N <= up["inner_path_steps"] <= c["n_outer"] * c["n_inner"] * N * (N + 1) // 2
    if not c["feller"] and c["scheme"] == 1:
        assert Yo.min() < 0.0  # the negative states the case is there for
