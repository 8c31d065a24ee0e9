"""What sub-optimality checking of the price bounds (option "bounds_suboptimality") offers without a GPU:
the frozen interface, the facades' signatures and argument checks, and the numpy restatement of
tests/helpers/bounds_check_ref.py on numpy paths -- the checked walk against the dense one, the kept sets, the step counts, the
lattice value under every mode's upper bound, the fuzz cases free of ties and of borderline items."""
import ctypes as C
import dataclasses
import functools
import inspect
import os

import numpy as np
import pytest

from helpers import bounds_check_ref as bk
from helpers import bounds_cv_ref as cv
from helpers import bounds_ref as br
from helpers import bounds_schedule_ref as bs
from options_model_amd import _ffi, api

K, R, SIG, T = 100.0, 0.05, 0.2, 1.0
N, N_OUTER, N_INNER = 12, 256, 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the interface
def test_interface_is_frozen_and_the_header_names_the_option():
    lib = _ffi.load_library()
    assert lib.omc_abi_version() == 14 == _ffi.ABI_VERSION
    assert len(_ffi.SIGNATURES) == 80
    assert C.sizeof(_ffi.BoundsConfig) == 2 * 4 + 3 * 8 + 3 * 8
    header = open(os.path.join(ROOT, "include", "omc.h")).read()
    assert '"bounds_suboptimality"' in header and "-40" in header
    knobs = header[header.index('"gbm_vec" / "heston_vec"') - 4000:header.index("int omc_set_option(")]
    assert '"bounds_suboptimality"' in knobs
    assert knobs.index('"bounds_control_variate"') < knobs.index('"bounds_suboptimality"')
    assert _ffi.BOUND_CHECKS == bk.MODES == ("off", "payoff", "european")


def test_facades_signatures_and_defaults():
    for fn in (_ffi.Context.price_american_bounds, _ffi.Context.price_american_bounds_heston,
               _ffi.Context.price_american_basket_bounds, api.price_american_basket_bounds):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "suboptimality_check" and last.default is None, fn
    # the pinned tails are unchanged
    assert list(inspect.signature(api.price_american_bounds).parameters)[-2:] == ["control_variate", "exercise_every"]
    assert list(inspect.signature(api.price_american_bounds_heston).parameters)[-2:] == ["regressors", "exercise_every"]
    assert list(inspect.signature(api.price_bermudan_bounds).parameters)[-1] == "control_variate"
    sig = inspect.signature(api.price_american_bounds_checked).parameters
    assert list(sig)[:9] == ["S0", "K", "r", "sigma", "T", "n_paths", "n_steps", "check", "model"]
    assert sig["check"].default == "european" and sig["model"].default == "GBM" and sig["control_variate"].default is False
    import options_model_amd
    assert options_model_amd.price_american_bounds_checked is api.price_american_bounds_checked
    for cls in (api.BoundsResult, api.HestonBoundsResult, api.BasketBoundsResult):
        assert {x.name: x.default for x in dataclasses.fields(cls)}["suboptimality_check"] == "off"


def test_facades_refuse_before_the_device():
    """no context is given and none is made (device 10^6 does not exist): the checks come first"""
    args = (100.0, K, R, SIG, T, 1000, 4)
    for bad in ("yes", 1, None, "European"):
        with pytest.raises(ValueError, match="check"):
            api.price_american_bounds_checked(*args, check=bad, device=10 ** 6)
    with pytest.raises(ValueError, match="european"):
        api.price_american_bounds_checked(*args, check="european", model="Heston", device=10 ** 6)
    with pytest.raises(ValueError, match="european"):
        api.price_american_bounds_checked(*args, model="Heston", device=10 ** 6)  # the default check is GBM's
    for k in (2, 5):
        with pytest.raises(ValueError, match="exercise_every"):
            api.price_american_bounds_checked(*args, check="payoff", exercise_every=k, device=10 ** 6)
    with pytest.raises(ValueError, match="model"):
        api.price_american_bounds_checked(*args, check="payoff", model="SABR", device=10 ** 6)
    with pytest.raises(ValueError, match="control_variate"):
        api.price_american_bounds_checked(*args, check="payoff", model="Heston", control_variate=True, device=10 ** 6)
    basket = ([100.0, 95.0], K, R, [0.2, 0.3], T, 1000, 4)
    with pytest.raises(ValueError, match="suboptimality_check"):
        api.price_american_basket_bounds(*basket, suboptimality_check="sometimes", device=10 ** 6)
    with pytest.raises(ValueError, match="european"):
        api.price_american_basket_bounds(*basket, suboptimality_check="european", device=10 ** 6)
    with pytest.raises(ValueError, match="suboptimality_check"):
        api.price_american_basket_bounds(*basket, kind="best-of", option_type="call", regressors="index+runner-up",
                                         suboptimality_check="payoff", device=10 ** 6)


# ------------------------------------------------------------------ the restatement on numpy paths
def _paths(n, rows, m, s0, seed):
    return bs.numpy_paths(dict(T=T, N=n, sigma=SIG, r=R), rows, m, s0, seed)


def _fitted(n, is_put, seed=3):
    """a policy fitted by plain least squares on numpy paths, classic Longstaff-Schwartz: [N+1][4] = b0, b1, b2, n"""
    S = _paths(n, n + 1, 20_000, 100.0, seed).astype(np.float64)
    D = cv.discounts(n, R, T)
    pay = (lambda s: np.maximum(K - s, 0.0)) if is_put else (lambda s: np.maximum(s - K, 0.0))
    cash, when = pay(S[n]), np.full(S.shape[1], n)
    betas = np.zeros((n + 1, 4))
    for t in range(n - 1, 0, -1):
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


CASES = [(is_put, S0) for is_put in (True, False) for S0 in (90.0, 100.0, 110.0)]
IDS = [f"{'put' if c[0] else 'call'}-{c[1]:.0f}" for c in CASES]


@functools.lru_cache(maxsize=None)
def _case(is_put, S0):
    """the outer paths, the inner paths' dense Q^ and every item's steps of a case, computed once and left unchanged"""
    betas = _fitted(N, is_put)
    So = _paths(N, N + 1, N_OUTER, S0, 21)
    seed0 = 1000 + int(S0)

    def inner(i, t):
        return _paths(N, N - t + 1, N_INNER, float(So[t, i]), seed0 + i * (N + 1) + t)

    rows = range(N_OUTER)
    dense = bk.item_steps(So, inner, rows, K, R, T, is_put, betas)  # one pass: bounds_ref.q_rows' values with every item's steps
    head = br.q_rows(So, inner, range(4), K, R, T, is_put, betas)
    assert dense["ties"] == 0 and int(dense["steps"][:4].sum()) == head["inner_path_steps"]
    np.testing.assert_array_equal(dense["q"][:4], head["q"])
    steps = dense
    walk = br.walk_rows(So, dense["q"], rows, K, R, T, is_put, betas)
    keeps = {m: bk.keep(So, betas, m, K, R, T, is_put, SIG) for m in (0, 1, 2)}
    for a in (So, dense["q"], steps["steps"], walk["samples"]):
        a.setflags(write=False)
    return dict(betas=betas, So=So, inner=inner, q=dense["q"], steps=steps["steps"], walk=walk, keeps=keeps,
                lattice=br.lattice(S0, K, R, SIG, T, N, is_put))


def _checked_q(c, m):
    """the dense Q^ at the kept items, 0.0 elsewhere: the bits of the kept items are the unchecked call's"""
    return np.where(c["keeps"][m]["keep"].T, c["q"], 0.0)


@pytest.mark.parametrize("is_put,S0", CASES, ids=IDS)
def test_every_item_kept_is_the_dense_walk(is_put, S0):
    c = _case(is_put, S0)
    kd = c["keeps"][0]
    assert kd["keep"].all() and kd["ties"] == 0
    wk = bk.walk_rows(c["So"], c["q"], range(N_OUTER), kd["keep"], K, R, T, is_put, c["betas"])
    np.testing.assert_allclose(wk["samples"], c["walk"]["samples"], rtol=0, atol=1e-12)
    assert not np.isnan(wk["M"]).any()


@pytest.mark.parametrize("is_put,S0", CASES, ids=IDS)
def test_checked_walk_against_the_dense_walk(is_put, S0):
    c = _case(is_put, S0)
    rows = range(N_OUTER)
    dense = bk.walk_rows(c["So"], c["q"], rows, c["keeps"][0]["keep"], K, R, T, is_put, c["betas"])
    tol = br.samples_atol(N, c["q"], dense["zmax"])
    for m in (1, 2):
        kd = c["keeps"][m]
        assert kd["ties"] == 0
        wk = bk.walk_rows(c["So"], _checked_q(c, m), rows, kd["keep"], K, R, T, is_put, c["betas"])
        seen = ~np.isnan(wk["M"])
        np.testing.assert_array_equal(seen[:, 1:N], kd["keep"].T[:, 1:])
        assert seen[:, N].all() and seen[:, 0].all()
        excess_M = float(np.max(np.abs(wk["M"][seen] - dense["M"][seen])))
        excess = float(np.max(wk["samples"] - dense["samples"]))
        print(f"mode {m}: kept-date M deviates {excess_M:.3e} (tolerance {tol:.3e}), largest sample excess {excess:.3e}")
        assert excess_M <= tol  # the dense increments between two kept dates telescope
        assert np.all(wk["samples"] <= dense["samples"] + tol)  # a maximum over fewer dates of the same walk


@pytest.mark.parametrize("is_put,S0", CASES, ids=IDS)
def test_kept_sets_are_nested_proper_subsets(is_put, S0):
    c = _case(is_put, S0)
    k1, k2 = c["keeps"][1]["keep"], c["keeps"][2]["keep"]
    assert np.all(k1[k2]) and k1[0].all() and k2[0].all()
    assert k2.sum() < k1.sum() < k1.size
    stops = np.array([br.stop_rule(c["So"][t], t, N, K, is_put, c["betas"])[0] for t in range(N)])
    assert np.all(k1[1:][stops[1:]]) and np.all(k2[1:][stops[1:]])  # a date at which the policy stops is kept
    share = [float(c["steps"][k.T].sum()) / float(c["steps"].sum()) for k in (k1, k2)]
    print(f"items kept {k1.mean():.3f} / {k2.mean():.3f}, inner steps kept {share[0]:.3f} / {share[1]:.3f}")


@pytest.mark.parametrize("is_put,S0", CASES, ids=IDS)
def test_kept_steps_are_the_dense_steps_less_the_skipped_items(is_put, S0):
    c = _case(is_put, S0)
    rows = range(32)
    for m in (1, 2):
        kp = c["keeps"][m]["keep"]
        got = bk.q_rows(c["So"], c["inner"], rows, kp, K, R, T, is_put, c["betas"])
        skipped = ~kp.T[:32]
        assert got["ties"] == 0
        assert got["inner_path_steps"] == int(c["steps"][:32].sum()) - int(c["steps"][:32][skipped].sum())
        np.testing.assert_array_equal(got["q"], _checked_q(c, m)[:32])  # the kept items' bits, 0.0 at the skipped ones


@pytest.mark.parametrize("is_put,S0", CASES, ids=IDS)
def test_upper_bound_stays_above_the_lattice(is_put, S0):
    c = _case(is_put, S0)
    ups = []
    for m in (0, 1, 2):
        kp = c["keeps"][m]["keep"]
        wk = bk.walk_rows(c["So"], _checked_q(c, m), range(N_OUTER), kp, K, R, T, is_put, c["betas"])
        up, se, _ = br._pair_mean_se(wk["samples"])
        ups.append(up)
        print(f"mode {m}: upper {up:.4f} (s.e. {se:.4f}), lattice {c['lattice']:.4f}")
        assert up >= c["lattice"] - 3 * se
    assert ups[2] <= ups[1] + 1e-9 and ups[1] <= ups[0] + 1e-9


@pytest.mark.parametrize("is_put", [True, False], ids=["put", "call"])
def test_a_never_exercising_table_counts_the_kept_items(is_put):
    c = _case(is_put, 100.0)
    never = np.zeros((N + 1, 4))
    kp = bk.keep(c["So"], never, 1, K, R, T, is_put)["keep"]
    x = c["So"][:N].astype(np.float64)
    np.testing.assert_array_equal(kp[1:], (((K - x) if is_put else (x - K)) > 0.0)[1:])  # nothing stops: the payoff alone
    rows = range(16)
    got = bk.q_rows(c["So"], c["inner"], rows, kp, K, R, T, is_put, never)
    want = N_INNER * sum(N - t for t in range(N) for i in rows if kp[t, i])
    assert got["inner_path_steps"] == want and 0 < want < N_INNER * 16 * N * (N + 1) // 2


# ------------------------------------------------------------------ the fuzz cases
def test_fuzz_cases_cover_what_they_promise():
    cases = bk.fuzz_cases(8)
    assert cases == bk.fuzz_cases(8) and cases == bk.fuzz_cases(12)[:8]  # seeded
    assert {c["model"] for c in cases} == set(bk.FUZZ_MODELS) and {c["mode"] for c in cases} == {1, 2}
    assert all(c["mode"] == 1 or c["model"].startswith("gbm") for c in cases)
    assert {c["n_inner"] for c in cases} == {16, 2, 64, 24, 192, 130, 10, 66}
    assert {c["is_put"] for c in cases} == {True, False} and len({c["policy"] for c in cases}) == 4
    assert all(c["n_outer"] % 2 == 0 and c["n_lower"] % 2 == 0 and c["M"] % 2 == 0 and 1 <= c["N"] <= 13 for c in cases)


@pytest.mark.parametrize("case", bk.fuzz_cases(8), ids=lambda c: f"{c['model']}-m{c['mode']}-N{c['N']}-i{c['n_inner']}")
def test_fuzz_case_restated_on_numpy_paths(case):
    """every case on numpy paths (one log-normal asset with the case's law): no stop tie, no borderline item, the checked
    samples at most the dense ones"""
    n, n_outer, n_inner = case["N"], min(case["n_outer"], 6), min(case["n_inner"], 32)
    is_put, r, sig, T_ = case["is_put"], case["r"], case["sigma"], case["T"]
    So = bs.numpy_paths(case, n + 1, n_outer, case["S0"], case["seed"] + 1)
    inner = lambda i, t: bs.numpy_paths(case, n - t + 1, n_inner, float(So[t, i]), case["seed"] + 7 + i * (n + 1) + t)  # noqa: E731
    rng = np.random.default_rng(case["seed"])
    betas = np.zeros((n + 1, 4))
    betas[1:n, 0], betas[1:n, 1], betas[1:n, 3] = rng.uniform(1.0, 9.0, n - 1), rng.uniform(-30.0, 30.0, n - 1), 40.0
    betas[np.asarray(case["holes"]), 3] = 0.0
    dense = bk.upper_bound(So, inner, 0, K, r, T_, is_put, betas)
    got = bk.upper_bound(So, inner, case["mode"], K, r, T_, is_put, betas, sigma=sig)
    assert dense["ties"] == 0 and got["ties"] == 0 and got["borderline"] == 0
    assert got["inner_path_steps"] <= dense["inner_path_steps"]
    np.testing.assert_array_equal(got["q"], np.where(got["keep"].T, dense["q"], 0.0))
    assert np.all(got["samples"] <= dense["samples"] + br.samples_atol(n, dense["q"], dense["zmax"]))
