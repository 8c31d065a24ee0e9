"""CPU suite of the multi-asset Greeks: the surface that needs no device, and the numpy restatement
(tests/helpers/basket_greeks_ref.py) -- each pathwise Greek against a central difference on common random numbers with
the exercise steps held, against the single-asset restatement for one asset, and the geometric kind's symmetry."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import basket_greeks_case as gc
from helpers import basket_greeks_ref as bgr
from helpers import basket_ref as br
from helpers import greeks_ref as gr
from oracle import cpu as orc

K, R, T = 100.0, 0.05, 1.0
KINDS = ("basket", "geometric", "best-of", "worst-of")
LAW = {2: dict(S0=[100.0, 96.0], sigma=[0.2, 0.3], q=[0.01, 0.03], rho=np.array([[1.0, 0.4], [0.4, 1.0]])),
       3: dict(S0=[100.0, 96.0, 104.0], sigma=[0.2, 0.25, 0.3], q=[0.01, 0.0, 0.03],
               rho=np.array([[1.0, 0.5, 0.2], [0.5, 1.0, -0.3], [0.2, -0.3, 1.0]]))}


def weights(d, kind):
    return ([0.6, 0.4] if d == 2 else [0.5, 0.3, 0.2]) if kind in ("basket", "geometric") else [1.0, 1.05, 0.95][:d]


def test_symbol_and_struct_are_bound_and_the_abi_stays():
    from options_model_amd import _ffi
    lib = _ffi.load_library()
    assert hasattr(lib, "omc_price_american_basket_greeks") and "omc_price_american_basket_greeks" in _ffi.SIGNATURES
    assert lib.omc_abi_version() == _ffi.ABI_VERSION == 14
    g = _ffi.BasketGreeks
    assert C.sizeof(g) == C.sizeof(_ffi.BasketResult) + 8 * (6 * 8 + 4 + 1 + 2 * 8 + 2 * 8 + 1) + 8
    assert g.delta.offset == C.sizeof(_ffi.BasketResult) and g.rho.offset == g.delta.offset + 6 * 64
    assert hasattr(_ffi.Context, "price_american_basket_greeks")


def test_facade_validates_without_a_device(monkeypatch):
    from options_model_amd import _ffi, api

    def no_device(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(_ffi, "default_context", no_device)
    monkeypatch.setattr(_ffi, "Context", no_device)
    args = ([100.0, 95.0], 100.0, 0.05, [0.2, 0.3], 1.0, 1000, 10)
    f = api.price_american_basket_greeks
    with pytest.raises(ValueError, match="one GPU"):
        f(*args, n_gpus=2)
    for bump in (0.0, 0.6, -0.1, float("nan")):
        with pytest.raises(ValueError, match="bump"):
            f(*args, bump=bump)
    with pytest.raises(ValueError, match="kind"):
        f(*args, kind="rainbow")
    with pytest.raises(ValueError):
        f([100.0, 95.0], 100.0, 0.05, [0.2], 1.0, 1000, 10)  # one sigma for two assets
    with pytest.raises(ValueError):
        f([100.0] * 9, 100.0, 0.05, [0.2] * 9, 1.0, 1000, 10)  # nine assets
    with pytest.raises(ValueError):
        f(*args, weights=[1.0])
    with pytest.raises(ValueError):
        f(*args, correlation=[[1.0, 0.2, 0.0], [0.2, 1.0, 0.0]])
    with pytest.raises(ValueError):
        f(*args, correlation=[[1.0, 2.0], [2.0, 1.0]])  # the library's own host check: not positive definite
    with pytest.raises(ValueError, match="betas"):
        f(*args, betas=np.zeros((10, 4)))
    with pytest.raises(ValueError):
        f(*args, option_type="straddle")
    with pytest.raises(ValueError):
        f([100.0, -95.0], 100.0, 0.05, [0.2, 0.3], 1.0, 1000, 10)
    import options_model_amd
    assert options_model_amd.price_american_basket_greeks is f and options_model_amd.BasketGreeksResult is api.BasketGreeksResult


# ------------------------------------------------------------------ float64 paths and their index
def _normals(d, N, P, seed):
    return np.random.default_rng(seed).standard_normal((d, N, P)).astype(np.float32)


def _index64(A, w, kind):
    """the index of float64 asset matrices with the float32 weights, nothing rounded (geometric: prod s_k^wf_k, which is
    G0 prod (s_k / S0_k)^wf_k)"""
    wd = np.asarray(w, np.float32).astype(np.float64)
    d = len(wd)
    if kind == "basket":
        return sum(wd[k] * A[k] for k in range(d))
    if kind == "geometric":
        return np.exp(sum(wd[k] * np.log(A[k]) for k in range(d)))
    P = np.stack([wd[k] * A[k] for k in range(d)])
    return P.max(axis=0) if kind == "best-of" else P.min(axis=0)


def _assets64(z, S0, sigma, q, L, r, T_):
    """basket_ref.assets with nothing rounded to float32: the step constants a_i, b_i, the factor L and the start spots stay
    float64.  (Through float32 constants a central difference in sigma_i, r or T carries their rounding, ulp(b) / eps ~ 1e-6
    relative: several of these paths' standard errors.)"""
    z = np.asarray(z, np.float64)
    d, N, P = z.shape
    dt = T_ / N
    out = np.empty((d, N + 1, 2 * P))
    for i in range(d):
        y = sum(L[i, k] * z[k] for k in range(i + 1))
        a, b = ((r - q[i]) - 0.5 * sigma[i] ** 2) * dt * br.L2E, sigma[i] * math.sqrt(dt) * br.L2E
        out[i, 0] = S0[i]
        out[i, 1:, :P] = S0[i] * np.exp2(np.cumsum(b * y + a, axis=0))
        out[i, 1:, P:] = S0[i] * np.exp2(np.cumsum(-b * y + a, axis=0))
    return out


def _paths(z, law, w, kind, r=R, T_=T, S0=None, sigma=None):
    S0 = law["S0"] if S0 is None else S0
    sigma = law["sigma"] if sigma is None else sigma
    A = _assets64(z, S0, sigma, law["q"], br.cholesky(law["rho"]), r, T_)
    return A, _index64(A, w, kind)


def _policy(X, is_put):
    ref = orc.lsm_poly(np.ascontiguousarray(X, np.float32), K, R, T, is_put, "two_pass")
    return gr.betas4_from(ref["betas"], ref["nitm"])


def _fixed_step_cf(X, r, T_, is_put, tex):
    """every path exercised at the step given for it, valued as the pricing values it"""
    N = X.shape[0] - 1
    x = X[tex, np.arange(X.shape[1])]
    return np.maximum(K - x if is_put else x - K, 0.0) * np.exp(-r * (T_ / N) * (tex - 1))


def _frozen_cf(X, r, T_, is_put, betas4):
    """the frozen policy applied to the index matrix X (float64): the latest firing step in 1 .. N-1, else N"""
    N, M = X.shape[0] - 1, X.shape[1]
    tex = np.full(M, N, np.int64)
    for t in range(N - 1, 0, -1):
        if betas4[t, 3] > 0.5:
            imm = K - X[t] if is_put else X[t] - K
            u = X[t] / K - 1.0
            ex = (tex == N) & (imm > 0.0) & (imm > u * (u * betas4[t, 2] + betas4[t, 1]) + betas4[t, 0])
            tex[ex] = t
    return _fixed_step_cf(X, r, T_, is_put, tex)


def _bumped(v, i, e):
    return [x + (e if j == i else 0.0) for j, x in enumerate(v)]


# (Greek, eps): the sizes tests/test_greeks_ref_cpu.py bumps by; theta is -dV/dT
EPS = {"delta": 0.5, "vega": 0.005, "rho": 0.002, "theta": 0.01}


def _central(name, i, z, law, w, kind, price):
    """-> (fd, t): the central difference at eps and eps / 2, Richardson-extrapolated (error O(eps^4)), and t, the mean
    truncation error of the plain central difference at eps that the extrapolation removes"""
    def fd(eps):
        cfs = []
        for e in (eps, -eps):
            kw = {"delta": dict(S0=_bumped(law["S0"], i, e)), "vega": dict(sigma=_bumped(law["sigma"], i, e)),
                  "rho": dict(r=R + e), "theta": dict(T_=T + e)}[name]
            _, Xb = _paths(z, law, w, kind, **kw)
            cfs.append(price(Xb, kw.get("r", R), kw.get("T_", T)))
        out = (cfs[0] - cfs[1]) / (2 * eps)
        return -out if name == "theta" else out

    coarse, fine = fd(EPS[name]), fd(EPS[name] / 2)
    star = (4.0 * fine - coarse) / 3.0
    return star, abs(float((coarse - star).mean()))


def _agree(term, value, fd, t, what):
    """tests/test_greeks_ref_cpu.py's statement and tolerance: the mean per-path difference within 4 of its standard errors
    (+ 1e-12 relative).  There the float32 rounding of the paths dominates the per-path differences; on float64 paths they
    are, away from the payoff's kink, the central difference's own smooth truncation error, whose mean no standard error
    covers.  So the reference is the extrapolated difference, and its residual truncation -- the square of the plain
    difference's relative error t / |value|, taken with a factor 10 -- is allowed for: of second order in an error that
    is itself of second order in eps, and far below the standard-error term wherever kink paths make t large."""
    d = term - fd
    se = d.std() / math.sqrt(len(d))
    floor = 10.0 * t * t / abs(value) if value != 0.0 else 0.0
    assert abs(d.mean()) <= 4 * se + 1e-12 * abs(value) + floor, (what, value, fd.mean(), se, floor)


def _check_all(g, d, z, law, w, kind, price):
    seen = {}
    for i in range(d):
        for name in ("delta", "vega"):
            _agree(g["terms"][name][i], g[name][i], *_central(name, i, z, law, w, kind, price), (name, i, kind))
            seen[name] = max(seen.get(name, 0.0), abs(g[name][i]) / g["se_" + name][i])
    for name in ("rho", "theta"):
        _agree(g["terms"][name], g[name], *_central(name, 0, z, law, w, kind, price), (name, kind))
        seen[name] = abs(g[name]) / g["se_" + name]
    # Greeks the check can see (a single asset's vega may legitimately vanish: its drift and diffusion effects cancel)
    assert all(v > 10.0 for v in seen.values()), seen


@pytest.mark.parametrize("is_put", [True, False])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [2, 3])
def test_pathwise_greeks_match_central_differences_at_held_exercise_steps(d, kind, is_put):
    """Fitted policy: every path keeps the exercise step the base chain gave it; the assets are regenerated from the same
    normals with one parameter bumped and the cash-flow is valued there.  That is the per-path derivative the kernel forms."""
    M, N = 20_000, 25
    law, w = LAW[d], weights(d, kind)
    z = _normals(d, N, M // 2, seed=17 + d)
    A, X = _paths(z, law, w, kind)
    g = bgr.greeks(A, X, K, R, T, is_put, _policy(X, is_put), law["S0"], law["sigma"], law["q"], w, kind, gamma=False)
    assert g["n_exercised"] < M and (g["n_exercised"] > 0 or not is_put)  # (a call on low yields may never exercise early)
    tex = g["tex"]
    _check_all(g, d, z, law, w, kind, lambda Xb, r, T_: _fixed_step_cf(Xb, r, T_, is_put, tex))


@pytest.mark.parametrize("is_put", [True, False])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [2, 3])
def test_pathwise_greeks_match_the_frozen_policy_central_difference_without_exercise(d, kind, is_put):
    """All-n = 0 table: the frozen-policy pricing has no decision boundary, so its central difference on regenerated paths
    and the pathwise Greek estimate the same derivative."""
    M, N = 20_000, 25
    law, w = LAW[d], weights(d, kind)
    z = _normals(d, N, M // 2, seed=29 + d)
    A, X = _paths(z, law, w, kind)
    b4 = np.zeros((N + 1, 4))
    g = bgr.greeks(A, X, K, R, T, is_put, b4, law["S0"], law["sigma"], law["q"], w, kind, gamma=False)
    assert g["n_exercised"] == 0
    _check_all(g, d, z, law, w, kind, lambda Xb, r, T_: _frozen_cf(Xb, r, T_, is_put, b4))


@pytest.mark.parametrize("is_put,K_", [(True, 100.0), (False, 95.0), (True, 110.0)])
@pytest.mark.parametrize("kind", KINDS)
def test_one_asset_is_the_single_asset_restatement(kind, is_put, K_):
    S0, sig, M, N, h = 100.0, 0.2, 20_000, 30, 0.01
    S = orc.gbm_paths(M, N, S0, R, sig, T, seed=5, stream=2)
    ref = orc.lsm_poly(S, K_, R, T, is_put, "two_pass")
    b4 = gr.betas4_from(ref["betas"], ref["nitm"])
    one = gr.greeks(S, K_, R, T, is_put, b4, S0, sig, h=h)
    g = bgr.greeks(S[None], S, K_, R, T, is_put, b4, [S0], [sig], [0.0], [1.0], kind, h=h)
    assert np.array_equal(g["tex"], one["tex"][0])
    for k in ("n_exercised", "n_zero"):
        assert g[k] == one[k], k
    assert (g["n_exercised_up"], g["n_exercised_down"]) == ([one["n_exercised_up"]], [one["n_exercised_down"]])

    def rel(a, b):
        return abs(a - b) <= 1e-12 * abs(b)

    for k in ("price", "rho", "theta", "se_rho", "se_theta"):
        assert rel(g[k], one[k]), (k, g[k], one[k])
    for k in ("delta", "gamma", "vega", "se_delta", "se_gamma", "se_vega", "price_up", "price_down"):
        assert rel(g[k][0], one[k]), (k, g[k], one[k])


@pytest.mark.parametrize("is_put", [True, False])
def test_geometric_deltas_are_proportional_to_the_weights(is_put):
    """x_i = wf_i X for every asset: delta_i S0_i / w_i is one number, path by path."""
    d, M, N = 3, 10_000, 12
    law, w = LAW[d], weights(d, "geometric")
    z = _normals(d, N, M // 2, seed=3)
    A, X = _paths(z, law, w, "geometric")
    g = bgr.greeks(A, X, K, R, T, is_put, _policy(X, is_put), law["S0"], law["sigma"], law["q"], w, "geometric", h=0.02)
    wf = np.asarray(w, np.float32).astype(np.float64)
    per_w = [g["delta"][i] * law["S0"][i] / wf[i] for i in range(d)]
    assert abs(per_w[0]) > 0.0
    for i in range(1, d):
        assert abs(per_w[i] - per_w[0]) <= 1e-13 * abs(per_w[0]), per_w
        np.testing.assert_allclose(g["terms"]["delta"][i] * law["S0"][i] / wf[i], g["terms"]["delta"][0] * law["S0"][0] / wf[0],
                                   rtol=1e-13, atol=0.0)


def test_fuzz_cases_are_deterministic_and_cover_the_ground():
    a, b = gc.fuzz_cases(12), gc.fuzz_cases(12)
    assert repr(a) == repr(b)
    assert {c["d"] for c in a} == set(range(1, 9)) and {c["kind"] for c in a} == set(gc.KINDS)
    assert all(1 <= c["N"] <= 70 and (c["M"] // 2) % 2 == 1 and 0.001 <= c["bump"] <= 0.5 for c in a)
    assert any(c["r"] == 0.0 for c in a) and any(c["given"] and any(c["holes"]) for c in a) and any(c["N"] == 1 for c in a)
    assert any(not c["gamma"] for c in a) and {c["is_put"] for c in a} == {True, False}
    assert repr(gc.fuzz_cases(3)) == repr(a[:3])
    for c in a:
        p, bk = gc.fuzz_params(c)
        assert (p.n_paths, p.n_steps, bk.n_assets) == (c["M"], c["N"], c["d"])
