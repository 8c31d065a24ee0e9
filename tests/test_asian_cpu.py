"""Asian (average-price) index kinds, OMC_BASKET_ASIAN_ARITHMETIC / _GEOMETRIC: what needs no GPU.

  1. the host table accepts the two kinds, codes 5 and 6 (x0 = sum w S0) -- on the library before these kinds this call
     returned -32; code 4 stays refused
  2. the numpy restatement (tests/helpers/asian_ref.py): its float32 fma against exact rational arithmetic, the arithmetic rule
     against a scalar loop, the float64 geometric rule against the product form
  3. the discrete geometric-average closed form against a float64 Monte Carlo of its own; arithmetic >= geometric
  4. the two-regressor stop rule on hand-written rows
  5. the facade's refusals, with no context made
  6. the interface is frozen: 80 entry points, ABI 14, the new kinds travel in omc_basket.kind
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from helpers import asian_ref as ar
from helpers import bounds_ref as br
from helpers import runnerup_ref as rr
from options_model_amd import _ffi


def _params(N=8, M=1000, is_put=True):
    return _ffi.make_params(model="gbm", is_put=is_put, semantics="two_pass", n_paths=M, n_steps=N, S0=100.0, K=100.0, r=0.05,
                            sigma=0.2, T=1.0, seed=1)


# ------------------------------------------------------------------ 1. the host table
@pytest.mark.parametrize("kind,code", [("asian", 5), ("asian-geometric", 6)])
def test_table_accepts_the_asian_kinds(kind, code):
    S0, w = [100.0, 90.0, 120.0], [0.5, 0.3, 0.2]
    b = _ffi.make_basket(S0, [0.2, 0.3, 0.25], [0.0, 0.01, 0.02], w, None, kind)
    assert int(b.kind) == code == _ffi.BASKET_KINDS[kind]
    L, a, bb, x0, geo = _ffi.basket_table(_params(), b)
    assert x0 == sum(wi * si for wi, si in zip(w, S0))  # X_0 = B_0
    plain = _ffi.basket_table(_params(), _ffi.make_basket(S0, [0.2, 0.3, 0.25], [0.0, 0.01, 0.02], w, None, "basket"))
    assert geo == plain[4] and x0 == plain[3]  # geo stays as for kind 0
    np.testing.assert_array_equal(a, plain[1])
    np.testing.assert_array_equal(bb, plain[2])


def test_unknown_kinds_stay_unknown():
    lib = _ffi.load_library()
    for k in (4, 7, 8, 9, -1):  # 4 was promised -32 before these kinds and keeps it
        b = _ffi.make_basket([100.0], [0.2], kind=k)
        assert lib.omc_basket_table(C.byref(_params()), C.byref(b), None, None, None, None, None) == -32


# ------------------------------------------------------------------ 2. the restatement
def test_fmaf32_is_one_rounding():
    rng = np.random.default_rng(7)
    a = rng.uniform(0.5, 2.0, 4000).astype(np.float32)
    b = rng.uniform(50.0, 200.0, 4000).astype(np.float32)
    c = rng.uniform(-300.0, 300.0, 4000).astype(np.float32)
    # cases whose float64 sum lands ON a float32 tie that the exact sum misses: a b = 0.5 - 2^-47, c = +-(2^23 + 1): a
    # float64 add followed by a float32 rounding goes to the even neighbour, one rounding goes to the odd one
    a[:3] = np.float32(1.0) + np.float32(2.0 ** -23)
    b[:3] = np.float32(0.5) - np.float32(2.0 ** -24)
    c[:3] = (2.0 ** 23 + 1.0, 2.0 ** 23 + 2.0, -(2.0 ** 23 + 1.0))
    naive = (a[:3].astype(np.float64) * b[:3].astype(np.float64) + c[:3].astype(np.float64)).astype(np.float32)
    assert (naive != ar.fmaf32(a[:3], b[:3], c[:3])).sum() == 2  # the cases do what they are there for
    got = ar.fmaf32(a, b, c)
    for i in range(400):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))  # float(Fraction) rounds once to float64; repair to one float32 rounding below
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i])


def test_arithmetic_rule_against_a_scalar_loop():
    rng = np.random.default_rng(11)
    d, N, M = 3, 9, 50
    A = rng.uniform(60.0, 160.0, (d, N + 1, M)).astype(np.float32)
    w = [0.5, 0.3, 0.2]
    X, B, c = ar.arithmetic_index(A, w)
    assert X.dtype == B.dtype == c.dtype == np.float32
    np.testing.assert_array_equal(X[0], B[0])
    assert not c[0].any()
    wf = np.asarray(w, np.float32)
    for j in range(M):
        run = np.float32(0.0)
        for t in range(1, N + 1):
            Bt = wf[0] * A[0, t, j]
            for k in (1, 2):
                Bt = ar.fmaf32(wf[k], A[k, t, j], Bt)
            assert Bt == B[t, j]
            run = np.float32(run + Bt)
            assert run == c[t, j] and X[t, j] == np.float32(run * (np.float32(1.0) / np.float32(t)))
    # continuing from a stored state is the same recurrence
    X2, c2 = ar.continue_arithmetic(B[5:], c[4], 4)
    np.testing.assert_array_equal(X2, X[5:])
    np.testing.assert_array_equal(c2, c[5:])
    # one date: the average is the basket value
    np.testing.assert_array_equal(ar.arithmetic_index(A[:, :2], w)[0], B[:2])


def test_geometric_rule_is_the_product_form():
    rng = np.random.default_rng(12)
    A = rng.uniform(60.0, 160.0, (2, 8, 40)).astype(np.float32)
    w = [0.6, 0.4]
    X = ar.geometric_index(A, w)
    B = ar.basket_value(A, w).astype(np.float64)
    for t in range(1, 8):
        np.testing.assert_allclose(X[t], np.prod(B[1:t + 1], axis=0) ** (1.0 / t), rtol=1e-13)
    Xa = ar.arithmetic_index(A, w)[0]
    assert (Xa[1:] >= X[1:] * (1 - 1e-6)).all()


# ------------------------------------------------------------------ 3. the closed form
MC = dict(S0=100.0, r=0.05, q=0.02, sigma=0.3, T=1.0, N=12)


@pytest.fixture(scope="module")
def mc_paths():
    return ar.gbm_paths64(np.random.default_rng(20261019), 400_000, **MC)


@pytest.mark.parametrize("is_put", [True, False])
@pytest.mark.parametrize("K", [90.0, 100.0, 110.0])
def test_closed_form_against_monte_carlo(mc_paths, K, is_put):
    G = np.exp(np.mean(np.log(mc_paths), axis=0))
    pay = np.maximum(K - G, 0.0) if is_put else np.maximum(G - K, 0.0)
    disc = math.exp(-MC["r"] * MC["T"])
    est, se = disc * pay.mean(), disc * pay.std(ddof=1) / math.sqrt(pay.size)
    cf = ar.geometric_asian_european(MC["S0"], K, MC["r"], MC["q"], MC["sigma"], MC["T"], MC["N"], is_put)
    print(f"K {K} put {is_put}: closed form {cf:.5f}  MC {est:.5f} ({se:.5f})")
    assert abs(est - cf) <= 4 * se
    m, v = ar.geometric_moments(MC["S0"], MC["r"], MC["q"], MC["sigma"], MC["T"], MC["N"])
    lg = np.log(G)
    assert abs(lg.mean() - m) <= 4 * math.sqrt(v / lg.size)
    assert abs(lg.var() / v - 1.0) <= 4 * math.sqrt(2.0 / lg.size)


def test_arithmetic_average_dominates_geometric(mc_paths):
    G = np.exp(np.mean(np.log(mc_paths), axis=0))
    A = np.mean(mc_paths, axis=0)
    assert (A >= G * (1.0 - 1e-14)).all()  # AM-GM, path by path
    disc = math.exp(-MC["r"] * MC["T"])
    for K in (90.0, 100.0, 110.0):
        assert disc * np.maximum(A - K, 0.0).mean() >= disc * np.maximum(G - K, 0.0).mean()
        cf = ar.geometric_asian_european(MC["S0"], K, MC["r"], MC["q"], MC["sigma"], MC["T"], MC["N"], False)
        se = disc * np.maximum(A - K, 0.0).std(ddof=1) / math.sqrt(A.size)
        assert disc * np.maximum(A - K, 0.0).mean() >= cf - 4 * se


# ------------------------------------------------------------------ 4. the two-regressor stop rule
def test_stop_rule_on_hand_written_rows():
    K, N = 100.0, 4
    X = np.array([90.0, 95.0, 99.0, 101.0], np.float32)  # the average
    B = np.array([80.0, 99.0, 120.0, 70.0], np.float32)  # the spot
    rows = np.zeros((N + 1, 8))
    # date 1: continuation 4 everywhere: the put stops where K - X > 4 and is in the money
    rows[1] = (4.0, 0, 0, 0, 0, 0, 10.0, 0)
    st, ties = rr.stop_rule(X, B, 1, N, K, True, rows)
    assert st.tolist() == [True, True, False, False] and ties == 0
    # ... which is the one-regressor rule of the same (c0, c1, c2, n)
    st4, _ = br.stop_rule(X, 1, N, K, True, np.array([[0, 0, 0, 0], [4.0, 0, 0, 10.0]] + [[0, 0, 0, 0]] * 3))
    assert st4.tolist() == st.tolist()
    # date 2: continuation 4 - 50 w, w = B / K - 1: a spot below the average (w < 0) makes waiting worth more
    rows[2] = (4.0, 0, 0, -50.0, 0, 0, 10.0, 0)
    st, ties = rr.stop_rule(X, B, 2, N, K, True, rows)
    #   cont = 4 + 10 = 14 > 10;  4 + 0.5 = 4.5 < 5;  4 - 10 = -6 < 1;  out of the money
    assert st.tolist() == [False, True, True, False] and ties == 0
    # the cross term: cont = 100 u w
    rows[3] = (0.0, 0, 0, 0, 0, 100.0, 10.0, 0)
    st, _ = rr.stop_rule(X, B, 3, N, K, True, rows)
    #   u = -.1 w = -.2: 2 < 10;  u = -.05 w = -.01: .05 < 5;  u = -.01 w = .2: -.2 < 1
    assert st.tolist() == [True, True, True, False]
    # n = 0: nobody exercises; date N: everybody stops
    rows[3, 6] = 0.0
    assert not rr.stop_rule(X, B, 3, N, K, True, rows)[0].any()
    assert rr.stop_rule(X, B, N, N, K, True, rows)[0].all()
    # a call: in the money above K only
    rows[1] = (0.5, 0, 0, 0, 0, 0, 3.0, 0)
    assert rr.stop_rule(X, B, 1, N, K, False, rows)[0].tolist() == [False, False, False, True]
    # a decision on the boundary is counted as a tie
    rows[1] = (5.0, 0, 0, 0, 0, 0, 3.0, 0)
    assert rr.stop_rule(X, B, 1, N, K, True, rows)[1] == 1


# ------------------------------------------------------------------ 5. refusals of the facade, no context made
def test_facade_refusals():
    from options_model_amd import price_american_basket_bounds
    from options_model_amd.api import price_asian_option

    assert not _ffi._default_ctx
    with pytest.raises(ValueError, match="averaging"):
        price_asian_option(100.0, 100.0, 0.05, 0.2, 1.0, 1000, 8, averaging="harmonic", device=10 ** 6)
    args = dict(spots=[100.0, 100.0], K=100.0, r=0.05, sigmas=[0.2, 0.2], T=1.0, n_paths=1000, n_steps=8, device=10 ** 6)
    with pytest.raises(ValueError, match="index\\+spot"):
        price_american_basket_bounds(kind="basket", regressors="index+spot", **args)
    with pytest.raises(ValueError, match="index\\+spot"):
        price_american_basket_bounds(kind="best-of", regressors="index+spot", **args)
    with pytest.raises(ValueError, match="runner-up"):
        price_american_basket_bounds(kind="asian", regressors="index+runner-up", **args)
    with pytest.raises(ValueError, match="512"):
        price_american_basket_bounds(kind="asian", regressors="index+spot", **dict(args, n_steps=513))
    with pytest.raises(ValueError, match="textbook"):
        price_american_basket_bounds(kind="asian", regressors="index+spot", policy="two_pass", **args)
    with pytest.raises(ValueError, match="bounds=True"):
        price_asian_option(100.0, 100.0, 0.05, 0.2, 1.0, 1000, 8, n_outer=64, device=10 ** 6)
    with pytest.raises(ValueError, match="kind"):
        price_american_basket_bounds(kind="lookback", **args)
    assert not _ffi._default_ctx  # nothing above made a context


def test_facade_is_exported():
    import options_model_amd
    from options_model_amd import api

    assert options_model_amd.price_asian_option is api.price_asian_option


# ------------------------------------------------------------------ 6. the frozen interface
def test_interface_is_frozen():
    names = sorted(_ffi.SIGNATURES)
    assert len(names) == 80
    assert not [n for n in names if "asian" in n or "lookback" in n or "average" in n]
    lib = _ffi.load_library()
    assert lib.omc_abi_version() == 14
    for n in ("omc_price_asian", "omc_price_american_asian", "omc_price_american_asian_bounds"):
        assert not hasattr(lib, n)
    assert C.sizeof(_ffi.Basket) == 8 + 8 * (4 * 8 + 64)  # no struct change
    assert {k: v for k, v in _ffi.BASKET_KINDS.items() if v < 4} == \
        {"basket": 0, "arithmetic": 0, "geometric": 1, "best-of": 2, "worst-of": 3}
