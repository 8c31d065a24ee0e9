"""What omc_price_american_basket_bounds_runnerup offers without a GPU: the symbol and the ABI version,
the facade's and the context method's argument checks, and the numpy restatement's own pieces (tests/helpers/runnerup_ref.py)
-- the runner-up on hand-written rows, the centred LDL' fit against numpy.linalg.lstsq, the truncation rule, the fuzz cases."""
import numpy as np
import pytest

from helpers import runnerup_ref as rr
from options_model_amd import _ffi, price_american_basket_bounds

K = 100.0


# ------------------------------------------------------------------ the interface
def test_symbol_and_abi_version():
    lib = _ffi.load_library()
    assert lib.omc_abi_version() == 14 == _ffi.ABI_VERSION
    assert lib.omc_price_american_basket_bounds_runnerup.restype is not None
    assert len(lib.omc_price_american_basket_bounds_runnerup.argtypes) == 9


@pytest.mark.parametrize("kw", [dict(kind="basket"), dict(kind="geometric"), dict(kind="best-of", spots=[100.0], sigmas=[0.2])],
                         ids=["basket", "geometric", "one-asset"])
def test_facade_refuses_before_the_device(kw):
    """no context is given and none is made: the checks come first"""
    args = dict(spots=[100.0, 100.0], K=K, r=0.05, sigmas=[0.2, 0.2], T=1.0, n_paths=1000, n_steps=4)
    args.update(kw)
    with pytest.raises(ValueError, match="runner-up"):
        price_american_basket_bounds(regressors="index+runner-up", device=10 ** 6, **args)


def test_facade_refuses_other_policies_and_regressors():
    args = dict(spots=[100.0, 100.0], K=K, r=0.05, sigmas=[0.2, 0.2], T=1.0, n_paths=1000, n_steps=4, kind="best-of",
                device=10 ** 6)
    for policy in ("two_pass", "reference"):
        with pytest.raises(ValueError, match="textbook"):
            price_american_basket_bounds(regressors="index+runner-up", policy=policy, **args)
    with pytest.raises(ValueError, match="regressors"):
        price_american_basket_bounds(regressors="index+third", **args)


def test_betas_shape_is_checked():
    """(N + 1, 8) with the runner-up, (N + 1, 4) without: raised by the context method before it calls the library"""
    ctx = object.__new__(_ffi.Context)  # never opened: the check needs no device
    ctx.handle = None
    N = 5
    p = _ffi.make_params(model="gbm", is_put=False, semantics="two_pass", n_paths=1000, n_steps=N, S0=100.0, K=K, r=0.05,
                         sigma=0.2, T=1.0, seed=1, stream=0)
    b = _ffi.make_basket([100.0, 100.0], [0.2, 0.2], None, [1.0, 1.0], None, "best-of")
    with pytest.raises(ValueError, match=r"\(6, 8\)"):
        ctx.price_american_basket_bounds(p, b, policy="given", betas=np.zeros((N + 1, 4)), regressors="index+runner-up")
    with pytest.raises(ValueError, match=r"\(6, 4\)"):
        ctx.price_american_basket_bounds(p, b, policy="given", betas=np.zeros((N + 1, 8)))
    with pytest.raises(ValueError, match="runner-up"):
        ctx.price_american_basket_bounds(p, _ffi.make_basket([100.0, 90.0], [0.2, 0.2]), regressors="index+runner-up")


# ------------------------------------------------------------------ the helper's runner-up
def test_runner_up_on_hand_written_rows():
    A = np.array([[3.0, 5.0, 2.0, 7.0], [4.0, 5.0, 9.0, 1.0], [1.0, 2.0, 9.0, 7.0]], np.float32)  # [d = 3][4 paths]
    X, Y = rr.xy(A, [1.0, 1.0, 1.0], "best-of")
    np.testing.assert_array_equal(X, [4.0, 5.0, 9.0, 7.0])
    np.testing.assert_array_equal(Y, [3.0, 5.0, 9.0, 7.0])  # ties count with multiplicity: Y = X
    X, Y = rr.xy(A, [1.0, 1.0, 1.0], "worst-of")
    np.testing.assert_array_equal(X, [1.0, 2.0, 2.0, 1.0])
    np.testing.assert_array_equal(Y, [3.0, 5.0, 9.0, 7.0])
    X, Y = rr.xy(A[:2], [2.0, 1.0], "best-of")  # d = 2: the runner-up is the other asset; weights are float32 factors
    np.testing.assert_array_equal(X, [6.0, 10.0, 9.0, 14.0])
    np.testing.assert_array_equal(Y, [4.0, 5.0, 4.0, 1.0])
    X, Y = rr.xy(A[:2], [1.0, 1.0], "worst-of")
    np.testing.assert_array_equal((X, Y), ([3.0, 5.0, 2.0, 1.0], [4.0, 5.0, 9.0, 7.0]))
    w = np.float32(1.1)
    X, _ = rr.xy(A[:2], [1.1, 1.1], "best-of")
    np.testing.assert_array_equal(X, np.maximum(w * A[0], w * A[1]))  # float32 products
    with pytest.raises(AssertionError):
        rr.xy(A, [1.0, 1.0, 1.0], "best-of", S=np.array([4.0, 5.0, 9.0, 7.5], np.float32))
    with pytest.raises(ValueError):
        rr.xy(A[:1], [1.0], "best-of")


def test_stop_rule_and_tie_band():
    N, t = 4, 2
    b = np.zeros((N + 1, 8))
    b[t] = (5.0, 0.0, 0.0, 10.0, 0.0, 0.0, 7.0, 0.0)  # cont = 5 + 10 w
    X = np.array([110.0, 110.0, 104.0, 99.0], np.float32)
    Y = np.array([100.0, 108.0, 90.0, 50.0], np.float32)  # cont = 5, 5.8, 4, .
    st, ties = rr.stop_rule(X, Y, t, N, K, False, b)
    np.testing.assert_array_equal(st[[0, 1, 3]], [True, True, False])  # imm = 10, 10, (4: a tie), out of the money
    assert ties == 1
    b[t][6] = 0.0
    assert not rr.stop_rule(X, Y, t, N, K, False, b)[0].any()  # nobody was in the money there: no exercise
    assert rr.stop_rule(X, Y, N, N, K, False, b)[0].all()


# ------------------------------------------------------------------ the helper's fit
def _regression_set(rng, n, d, kind):
    A = (100.0 * np.exp(rng.normal(0.0, 0.25, (d, n)))).astype(np.float32)
    X, Y = rr.xy(A, np.ones(d), kind)
    u, w = rr.uw(X, Y, K)
    y = np.maximum(8.0 + 30.0 * u - 12.0 * w + 20.0 * u * w + rng.normal(0.0, 6.0, n), 0.0)
    return u, w, y


@pytest.mark.parametrize("n", [20, 300, 5000, 100_000])
def test_ldl_fit_equals_lstsq(n):
    """fitted values on the set within 1e-9 K of numpy's SVD solve (measured: at most 8.1e-11 at K = 100 over 40 sets)"""
    worst = 0.0
    for s in range(10 if n < 100_000 else 3):
        rng = np.random.default_rng(1000 * n + s)
        d = 2 + (s + n) % 7
        u, w, y = _regression_set(rng, n, d, rr.KINDS[s % 2])
        row = rr.ldl_fit(u, w, y)
        G = np.stack([np.ones(n), u, u * u, w, w * w, u * w], axis=1)
        coef = np.linalg.lstsq(G, y, rcond=None)[0]
        assert row[6] == n and row[7] == 0.0
        diff = float(np.max(np.abs(G @ coef - rr.continuation(u, w, row))))
        worst = max(worst, diff)
        assert diff <= 1e-9 * K, (n, s, d, diff)
    print(f"n = {n}: largest difference of fitted values {worst:.3g}")


def test_ldl_fit_truncates_a_constant_runner_up():
    """all Y equal: the centred w column is zero, so w and every later feature (w^2, uw) get coefficient 0 and what is left is
    the quadratic in u"""
    rng = np.random.default_rng(7)
    u, _, y = _regression_set(rng, 500, 3, "best-of")
    w = np.full(500, -0.125)
    row = rr.ldl_fit(u, w, y)
    assert not row[3:6].any() and row[6] == 500
    coef = np.linalg.lstsq(np.stack([np.ones(500), u, u * u], axis=1), y, rcond=None)[0]
    np.testing.assert_allclose(row[:3], coef, rtol=1e-9, atol=1e-9)
    # fewer rows than coefficients: n = 2 keeps one feature, n = 1 the mean, n = 0 nothing
    r2 = rr.ldl_fit(np.array([0.1, 0.2]), np.array([0.0, 0.05]), np.array([3.0, 5.0]))
    assert r2[6] == 2 and not r2[2:6].any() and np.allclose(r2[:2], (1.0, 20.0))
    r1 = rr.ldl_fit(np.array([0.1]), np.array([0.0]), np.array([3.0]))
    assert r1[0] == 3.0 and not r1[1:6].any() and r1[6] == 1
    assert not rr.ldl_fit(np.zeros(0), np.zeros(0), np.zeros(0)).any()


# ------------------------------------------------------------------ the fuzz cases
def test_fuzz_cases_cover_what_they_promise():
    cases = rr.fuzz_cases(12)
    for a, b in zip(cases, rr.fuzz_cases(12)):  # seeded: the same cases every time
        assert np.array_equal(a.pop("rho"), b["rho"]) and a == {k: v for k, v in b.items() if k != "rho"}
    cases = rr.fuzz_cases(12)
    assert {c["d"] for c in cases} == set(range(2, 9))
    assert {c["kind"] for c in cases} == set(rr.KINDS)
    assert all(1 <= c["N"] <= 13 and c["n_inner"] in rr.N_INNER and c["n_outer"] % 2 == 0 for c in cases)
    assert {c["n_inner"] for c in cases} >= {64, 130, 200} and len({c["n_outer"] for c in cases}) > 3
    assert 3 * sum(c["refill"] for c in cases) >= len(cases)
    given = [c for c in cases if c["policy"] == "given"]
    assert len(given) == len(cases) // 3 and all(len(c["holes"]) == c["N"] + 1 for c in cases)
    assert any(any(c["holes"][1:c["N"]]) for c in given)
    assert {c["is_put"] for c in cases} == {True, False}
    for c in cases:  # the library accepts every basket (host-side checks only)
        p, b = rr_params(c)
        assert _ffi.basket_table(p, b) is not None


def rr_params(case):
    from helpers import basket_bounds_case as bc

    return bc.fuzz_params(case)
