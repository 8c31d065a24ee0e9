"""What the Black-Scholes control variate of the GBM price bounds (option "bounds_control_variate")
offers without a GPU: the frozen interface, the facades' signatures and argument checks, and the numpy restatement of
tests/helpers/bounds_cv_ref.py on float64-driven numpy paths -- the control's mean, the identity with the plain estimator, the
exact zeros of a never-exercising table, E against bounds_ref.black_scholes, the variance ratios, the fuzz cases tie-free."""
import ctypes as C
import dataclasses
import inspect
import math
import os

import numpy as np
import pytest

from helpers import bounds_cv_ref as cv
from helpers import bounds_ref as br
from helpers import bounds_schedule_ref as bs
from options_model_amd import _ffi, api

K, R, SIG, T = 100.0, 0.05, 0.2, 1.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the interface
def test_interface_is_frozen_and_the_header_names_the_option():
    lib = _ffi.load_library()
    assert lib.omc_abi_version() == 14 == _ffi.ABI_VERSION
    assert len(_ffi.SIGNATURES) == 80
    assert C.sizeof(_ffi.BoundsConfig) == 2 * 4 + 3 * 8 + 3 * 8
    header = open(os.path.join(ROOT, "include", "omc.h")).read()
    assert '"bounds_control_variate"' in header and "-39" in header
    knobs = header[header.index('"gbm_vec" / "heston_vec"') - 4000:header.index("int omc_set_option(")]
    assert '"bounds_control_variate"' in knobs


def test_facades_signatures_and_defaults():
    names = list(inspect.signature(api.price_american_bounds).parameters)
    assert names[-2:] == ["control_variate", "exercise_every"]  # the schedule stays last
    assert inspect.signature(api.price_american_bounds).parameters["control_variate"].default is False
    last = list(inspect.signature(api.price_bermudan_bounds).parameters.values())[-1]
    assert last.name == "control_variate" and last.default is False
    assert inspect.signature(_ffi.Context.price_american_bounds).parameters["control_variate"].default is False
    for fn in (api.price_american_bounds_heston, api.price_american_basket_bounds, _ffi.Context.price_american_bounds_heston,
               _ffi.Context.price_american_basket_bounds):
        assert "control_variate" not in inspect.signature(fn).parameters
    f = {x.name: x.default for x in dataclasses.fields(api.BoundsResult)}
    assert f["control_variate"] is False


def test_facades_refuse_before_the_device():
    """no context is given and none is made (device 10^6 does not exist): the checks come first"""
    with pytest.raises(ValueError, match="control_variate"):
        api.price_bermudan_bounds(100.0, K, R, SIG, T, 1000, 4, 2, model="Heston", device=10 ** 6, control_variate=True)
    for bad in (2, "yes", None, 0.5):
        with pytest.raises(ValueError, match="control_variate"):
            api.price_american_bounds(100.0, K, R, SIG, T, 1000, 4, device=10 ** 6, control_variate=bad)
        with pytest.raises(ValueError, match="control_variate"):
            api.price_bermudan_bounds(100.0, K, R, SIG, T, 1000, 4, 2, device=10 ** 6, control_variate=bad)


# ------------------------------------------------------------------ E
@pytest.mark.parametrize("is_put", [True, False])
def test_euro_is_black_scholes(is_put):
    N = 12
    for x in (60.0, 99.5, 100.0, 131.25):
        for d in (0, 5, N - 1):
            want = br.black_scholes(x, K, R, SIG, (N - d) * (T / N), is_put)
            assert float(cv.euro(x, d, N, K, R, SIG, T, is_put)) == pytest.approx(want, rel=1e-14, abs=1e-14 * K)
    x = np.array([[80.0, 100.0], [120.0, 95.0]], np.float32)
    d = np.array([[0, 3], [11, 7]])
    got = cv.euro(x, d, N, K, R, SIG, T, is_put)
    for idx in np.ndindex(2, 2):
        assert got[idx] == float(cv.euro(x[idx], int(d[idx]), N, K, R, SIG, T, is_put))
    assert cv.e0(100.0, N, K, R, SIG, T, is_put) == pytest.approx(br.black_scholes(100.0, K, R, SIG, T, is_put), rel=1e-14)


# ------------------------------------------------------------------ the estimators on numpy paths
def _paths(N, rows, m, s0, seed):
    return bs.numpy_paths(dict(T=T, N=N, sigma=SIG, r=R), rows, m, s0, seed)


def _fitted(N, is_put, seed=3):
    """a policy fitted by plain least squares on numpy paths, classic Longstaff-Schwartz: [N+1][4] = b0, b1, b2, n"""
    S = _paths(N, N + 1, 20_000, 100.0, seed).astype(np.float64)
    D = cv.discounts(N, R, T)
    pay = (lambda s: np.maximum(K - s, 0.0)) if is_put else (lambda s: np.maximum(s - K, 0.0))
    cash, when = pay(S[N]), np.full(S.shape[1], N)
    betas = np.zeros((N + 1, 4))
    for t in range(N - 1, 0, -1):
        imm = pay(S[t])
        itm = imm > 0.0
        if itm.sum() < 10:
            continue
        u = S[t][itm] / K - 1.0
        y = cash[itm] * D[when[itm]] / D[t]
        coef = np.polyfit(u, y, 2)
        betas[t] = [coef[2], coef[1], coef[0], float(itm.sum())]
        ex = np.zeros_like(itm)
        ex[itm] = imm[itm] > np.polyval(coef, u)
        cash[ex], when[ex] = imm[ex], t
    if not is_put:  # a call without dividends is never exercised early: a rule that undervalues waiting, so that some paths stop
        betas[:, :3] *= 0.97
    return betas


@pytest.mark.parametrize("is_put", [True, False], ids=["put", "call"])
@pytest.mark.parametrize("k", [0, 3])
def test_the_control_has_mean_zero(is_put, k):
    """mean(D_tau E(S_tau, tau)) - E0 within 4 standard errors, on float32 paths driven by float64 normals"""
    N, n = 12, 40_000
    betas = _fitted(N, is_put)
    S = _paths(N, N + 1, n, 100.0, 11 + k)
    tau, x, Z, ties = cv.stopped(S, 0, N, K, R, T, is_put, bs.mask(betas, k))
    assert ties == 0 and 0 < np.count_nonzero(tau < N) < n  # the policy does stop early, and not everywhere
    ctl = cv.control(tau, x, Z, N, K, R, SIG, T, is_put)
    mean, se, _ = br._pair_mean_se(ctl)
    E0 = cv.e0(100.0, N, K, R, SIG, T, is_put)
    print(f"control mean {mean:.6f}, E0 {E0:.6f}, se {se:.6f}")
    assert abs(mean - E0) <= 4 * se
    c = cv.terms(tau, x, Z, N, K, R, SIG, T, is_put)
    assert np.all(c[tau == N] == 0.0) and np.array_equal(c[tau < N], (Z - ctl)[tau < N])


@pytest.mark.parametrize("is_put", [True, False], ids=["put", "call"])
@pytest.mark.parametrize("k", [0, 3])
def test_q_identity_with_the_plain_estimator(is_put, k):
    """q_cv = q_plain - mean(control) + D_t E_t, against bounds_ref.q_rows / bounds_schedule_ref.q_rows, to 1e-13 absolute"""
    N, n_outer, n_inner = 8, 6, 32
    betas = _fitted(N, is_put)
    So = _paths(N, N + 1, n_outer, 100.0, 21)
    items = {(i, t): _paths(N, N - t + 1, n_inner, float(So[t, i]), 100 + i * (N + 1) + t) for i in range(n_outer) for t in range(N)}
    inner = lambda i, t: items[(i, t)]  # noqa: E731
    rows = range(n_outer)
    got = cv.q_rows(So, inner, rows, K, R, SIG, T, is_put, betas, k)
    plain = (bs.q_rows(So, inner, rows, K, R, T, is_put, betas, k) if k else br.q_rows(So, inner, rows, K, R, T, is_put, betas))
    assert got["ties"] == plain["ties"] == 0 and got["inner_path_steps"] == plain["inner_path_steps"]
    np.testing.assert_array_equal(got["q_plain"], plain["q"])
    D = cv.discounts(N, R, T)
    bk = bs.mask(betas, k)
    for i in rows:
        for t in bs.schedule(N, k)[:-1]:
            tau, x, Z, _ = cv.stopped(inner(i, t), t, N, K, R, T, is_put, bk)
            ctl = cv.control(tau, x, Z, N, K, R, SIG, T, is_put)
            want = plain["q"][i, t] - ctl.mean() + D[t] * float(cv.euro(So[t, i], t, N, K, R, SIG, T, is_put))
            assert abs(got["q"][i, t] - want) <= 1e-13
    off = [t for t in range(N) if t not in bs.schedule(N, k)[:-1]]
    assert np.all(got["q"][:, off] == 0.0)


@pytest.mark.parametrize("k", [0, 3, 20])
def test_a_never_exercising_table_gives_zero_terms(k):
    N = 8
    S = _paths(N, N + 1, 64, 100.0, 5)
    lo = cv.lower_bound(S, K, R, SIG, T, True, np.zeros((N + 1, 4)), k)
    assert np.all(lo["c"] == 0.0) and lo["se_lower"] == 0.0 and lo["lower"] == lo["e0"] and lo["n_exercised"] == 0
    So = _paths(N, N + 1, 4, 100.0, 6)
    inner = lambda i, t: _paths(N, N - t + 1, 8, float(So[t, i]), 9 + i * (N + 1) + t)  # noqa: E731
    up = cv.upper_bound(So, inner, K, R, SIG, T, True, np.zeros((N + 1, 4)), k)
    want = cv.never_exercising(So, K, R, SIG, T, True, k)
    np.testing.assert_array_equal(up["q"], want["q"])
    np.testing.assert_allclose(up["samples"], want["samples"], rtol=0, atol=br.samples_atol(N, up["q"], up["zmax"]))
    if k >= N:
        np.testing.assert_allclose(up["samples"], want["q"][:, 0], rtol=0, atol=1e-12 * K)


def test_variance_ratios_are_above_one():
    """plain over controlled, on the restatement: the lower bound's pair means and the inner paths of the item at t = 0"""
    N, n = 12, 40_000
    betas = _fitted(N, True)
    S = _paths(N, N + 1, n, 100.0, 31)
    lo = cv.lower_bound(S, K, R, SIG, T, True, betas)
    P = n // 2
    vp = np.var(0.5 * (lo["Z"][:P] + lo["Z"][P:]))
    vc = np.var(0.5 * (lo["c"][:P] + lo["c"][P:]))
    Si = _paths(N, N + 1, 4096, 100.0, 32)
    tau, x, Z, _ = cv.stopped(Si, 0, N, K, R, T, True, betas)
    c = cv.terms(tau, x, Z, N, K, R, SIG, T, True)
    vpi = np.var(0.5 * (Z[:2048] + Z[2048:]))
    vci = np.var(0.5 * (c[:2048] + c[2048:]))
    print(f"variance ratio plain / controlled: lower bound {vp / vc:.1f}, item at t = 0 {vpi / vci:.1f}")
    assert vp / vc > 1.0 and vpi / vci > 1.0


# ------------------------------------------------------------------ the fuzz cases
def test_fuzz_cases_cover_what_they_promise():
    cases = cv.fuzz_cases(8)
    assert cases == cv.fuzz_cases(8) and cases == cv.fuzz_cases(12)[:8]  # seeded
    assert [c["k"] >= 2 for c in cases] == [i % 3 == 2 for i in range(8)]  # every third with a schedule
    assert {c["n_inner"] for c in cases} == {2, 16, 24, 64, 66, 192, 10, 130}
    assert {c["is_put"] for c in cases} == {True, False} and len({c["policy"] for c in cases}) == 4
    assert all(c["n_outer"] % 2 == 0 and c["n_lower"] % 2 == 0 and c["M"] % 2 == 0 and 1 <= c["N"] <= 13 for c in cases)


@pytest.mark.parametrize("case", cv.fuzz_cases(8), ids=lambda c: f"N{c['N']}-k{c['k']}-i{c['n_inner']}")
def test_fuzz_case_restated_on_numpy_paths(case):
    """every case on numpy paths: no tie, the same stops as the plain restatement, exact zeros where both partners reach N"""
    N, k, n_outer, n_inner = case["N"], case["k"], min(case["n_outer"], 6), min(case["n_inner"], 32)
    is_put, r, sig, T_ = case["is_put"], case["r"], case["sigma"], case["T"]
    Sl = bs.numpy_paths(case, N + 1, 400, case["S0"], case["seed"])
    So = bs.numpy_paths(case, N + 1, n_outer, case["S0"], case["seed"] + 1)
    inner = lambda i, t: bs.numpy_paths(case, N - t + 1, n_inner, float(So[t, i]), case["seed"] + 7 + i * (N + 1) + t)  # noqa: E731
    rng = np.random.default_rng(case["seed"])
    betas = np.zeros((N + 1, 4))
    betas[1:N, 0], betas[1:N, 1], betas[1:N, 3] = rng.uniform(1.0, 9.0, N - 1), rng.uniform(-30.0, 30.0, N - 1), 40.0
    betas[np.asarray(case["holes"]), 3] = 0.0
    lo = cv.lower_bound(Sl, K, r, sig, T_, is_put, betas, k)
    up = cv.upper_bound(So, inner, K, r, sig, T_, is_put, betas, k)
    assert lo["ties"] == 0 and up["ties"] == 0
    plo = bs.lower_bound(Sl, K, r, T_, is_put, betas, k)
    pup = bs.upper_bound(So, inner, K, r, T_, is_put, betas, k)
    assert lo["n_exercised"] == plo["n_exercised"] and up["inner_path_steps"] == pup["inner_path_steps"]
    np.testing.assert_array_equal(up["q_plain"], pup["q"])
    assert math.isfinite(lo["lower"]) and np.all(np.isfinite(up["q"])) and np.all(np.isfinite(up["samples"]))
