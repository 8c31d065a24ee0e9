"""What the price bounds of a game with an exercise schedule (option "bounds_exercise_every") offer
without a GPU: the frozen interface, the facades' argument checks, the schedule helper on hand cases, the numpy scheduled walk
of tests/helpers/bounds_schedule_ref.py against bounds_ref's all-dates walk, and the fuzz cases restated on numpy paths."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from helpers import bounds_ref as br
from helpers import bounds_schedule_ref as bs
from helpers import heston_bounds_case as hc
from options_model_amd import _ffi, api

K, R, T = 100.0, 0.05, 1.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the interface
def test_interface_is_frozen_and_the_header_names_the_option():
    lib = _ffi.load_library()
    assert lib.omc_abi_version() == 14 == _ffi.ABI_VERSION
    assert len(_ffi.SIGNATURES) == 80
    # policy, regressors, three sizes, three streams: no room was made for the schedule
    assert C.sizeof(_ffi.BoundsConfig) == 2 * 4 + 3 * 8 + 3 * 8
    header = open(os.path.join(ROOT, "include", "omc.h")).read()
    assert '"bounds_exercise_every"' in header and "-38" in header
    knobs = header[header.index('"gbm_vec" / "heston_vec"') - 4000:header.index("int omc_set_option(")]
    assert '"bounds_exercise_every"' in knobs and "GAME" in knobs


def test_facades_take_the_schedule_last_and_results_carry_it():
    import inspect

    for fn in (api.price_american_bounds, api.price_american_bounds_heston):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "exercise_every" and last.default == 0
    for fn in (_ffi.Context.price_american_bounds, _ffi.Context.price_american_bounds_heston):
        assert inspect.signature(fn).parameters["exercise_every"].default == 0
    import options_model_amd

    assert options_model_amd.price_bermudan_bounds is api.price_bermudan_bounds
    f = {x.name: x.default for x in dataclasses.fields(api.BoundsResult)}
    assert f["exercise_every"] == 0 and f["n_exercise_dates"] == 0
    assert {"exercise_every", "n_exercise_dates"} <= {x.name for x in dataclasses.fields(api.HestonBoundsResult)}


BAD = [(-1, "exercise_every"), (2.5, "exercise_every"), ([2, 3], "exercise_every"), ("2", "exercise_every"),
       (True, "exercise_every"), (None, "exercise_every"), (2 ** 31, "exercise_every")]


@pytest.mark.parametrize("every,match", BAD, ids=[repr(b[0]) for b in BAD])
@pytest.mark.parametrize("which", ["gbm", "heston", "bermudan-gbm", "bermudan-heston"])
def test_facades_refuse_before_the_device(which, every, match):
    """no context is given and none is made (device 10^6 does not exist): the checks come first"""
    with pytest.raises(ValueError, match=match):
        if which == "gbm":
            api.price_american_bounds(100.0, K, R, 0.2, T, 1000, 4, device=10 ** 6, exercise_every=every)
        elif which == "heston":
            api.price_american_bounds_heston(100.0, K, R, T, 1000, 4, heston_params=hc.HP, device=10 ** 6,
                                             exercise_every=every)
        else:
            api.price_bermudan_bounds(100.0, K, R, 0.2, T, 1000, 4, every, model=which.split("-")[1], device=10 ** 6)


def test_spot_variance_policy_refuses_a_schedule_before_the_device():
    with pytest.raises(ValueError, match="schedule"):
        api.price_american_bounds_heston(100.0, K, R, T, 1000, 4, heston_params=hc.HP, device=10 ** 6,
                                         regressors="spot+variance", exercise_every=2)
    with pytest.raises(ValueError, match="model"):
        api.price_bermudan_bounds(100.0, K, R, 0.2, T, 1000, 4, 2, model="merton", device=10 ** 6)


# ------------------------------------------------------------------ the schedule
def test_schedule_on_hand_cases():
    N = 12
    assert bs.schedule(N, 0) == bs.schedule(N, 1) == list(range(13))
    assert bs.schedule(N, 2) == [0, 2, 4, 6, 8, 10, 12]
    assert bs.schedule(N, 5) == [0, 2, 7, 12]           # N % k != 0: a short first gap
    assert bs.schedule(N, N - 1) == [0, 1, 12]
    assert bs.schedule(N, N) == [0, 12] == bs.schedule(N, N + 3)
    assert bs.schedule(7, 3) == [0, 1, 4, 7] and bs.schedule(1, 2) == [0, 1] and bs.schedule(1, 0) == [0, 1]
    for N in range(1, 15):
        for k in range(0, N + 4):
            taus = bs.schedule(N, k)
            J = len(taus) - 1
            assert taus[1:] == api.bounds_exercise_dates(N, k)
            assert taus[1:-1] == api.exercise_dates(N, k) and taus[-1] == N   # the chain's anchoring plus the expiry
            if k >= 2:
                assert J == (N - 1) // k + 1 == bs.n_dates(N, k)
                assert taus[1:] == [N - (J - j) * k for j in range(1, J + 1)]
                assert 1 <= taus[1] <= k
                assert bs.horizon(T, N, k) == (T if J * k == N else T * float(J * k) / float(N))
    assert bs.horizon(2.0, 12, 5) == 2.0 * 15.0 / 12.0 and bs.horizon(2.0, 12, 4) == 2.0 and bs.horizon(2.0, 12, 15) == 2.0 * 15 / 12
    with pytest.raises(ValueError):
        bs.schedule(5, -1)
    with pytest.raises(ValueError):
        api.bounds_exercise_dates(5, -1)
    assert bs.max_inner_steps(12, 5, 3, 4) == 3 * 4 * (12 + 10 + 5)
    assert bs.max_inner_steps(12, 1, 3, 4) == 3 * 4 * 12 * 13 // 2


def test_mask_and_gather():
    b = np.arange(1, 4 * 13 + 1, dtype=np.float64).reshape(13, 4)
    m = bs.mask(b, 5)
    assert np.all(m[[2, 7, 12]] == b[[2, 7, 12]]) and np.all(np.delete(m, [2, 7, 12], axis=0) == 0.0)
    assert np.all(bs.mask(b, 1) == b) and np.all(bs.mask(b, 0) == b)
    S = np.arange(13 * 3, dtype=np.float32).reshape(13, 3)
    assert np.all(bs.gather(S, 5) == S[[0, 2, 7, 12]]) and np.all(bs.gather(S, 0) == S)


# ------------------------------------------------------------------ the walk
def _walk_case(seed, N, n=24, is_put=True):
    rng = np.random.default_rng(seed)
    case = dict(T=T, N=N, sigma=0.3, r=R)
    So = bs.numpy_paths(case, N + 1, n, 100.0, seed)
    q = rng.uniform(0.0, 12.0, (n, N))
    betas = np.zeros((N + 1, 4))
    betas[1:N, 0] = rng.uniform(2.0, 9.0, N - 1)  # exercise when imm > b0 + b1 u
    betas[1:N, 1] = rng.uniform(-20.0, 0.0, N - 1)
    betas[1:N, 3] = 50.0
    return So, q, betas


@pytest.mark.parametrize("N", [1, 7, 12, 13])
def test_walk_every_date_is_bounds_refs(N):
    So, q, betas = _walk_case(5 + N, N)
    rows = range(So.shape[1])
    want = br.walk_rows(So, q, rows, K, R, T, True, betas)
    for k in (0, 1):
        got = bs.walk_rows(So, q, rows, K, R, T, True, betas, k)
        assert np.array_equal(got["samples"], want["samples"]) and got["ties"] == want["ties"] and got["zmax"] == want["zmax"]


@pytest.mark.parametrize("N,k", [(7, 2), (7, 3), (8, 5), (12, 5), (12, 11), (13, 3), (13, 6), (12, 4)])
def test_walk_telescopes_over_the_gaps(N, k):
    """With the policy holed to the schedule the all-dates walk adds Q_t - Q_{t-1} on every date off it, so its M at a
    scheduled date is the scheduled walk's (to rounding: 1e-12 of the values summed), and the scheduled sample, a maximum over
    fewer dates, never exceeds the all-dates one."""
    So, q, betas = _walk_case(100 * N + k, N)
    rows = range(So.shape[1])
    taus = bs.schedule(N, k)
    holed = bs.mask(betas, k)
    got = bs.walk_rows(So, q, rows, K, R, T, True, betas, k)
    assert np.array_equal(got["samples"], bs.walk_rows(So, q, rows, K, R, T, True, holed, k)["samples"])  # the mask is idempotent
    D = np.exp(-R * (T / N) * np.arange(N + 1))
    exercised = 0
    for m, i in enumerate(rows):  # the all-dates walk, M kept
        M, best = 0.0, -np.inf
        for t in range(1, N + 1):
            s = So[t, i:i + 1]
            Zt = D[t] * max(K - float(s[0]), 0.0)
            st, _ = br.stop_rule(s, t, N, K, True, holed)
            exercised += int(st[0] and t < N)
            qt = q[m, t] if t < N else 0.0
            M = M + (Zt if st[0] else qt) - q[m, t - 1]
            best = max(best, Zt - M)
            if t in taus:
                assert abs(M - got["M"][m, taus.index(t)]) <= 1e-12 * 12.0 * (N + 1)
        assert best == br.walk_rows(So, q[m:m + 1], [i], K, R, T, True, holed)["samples"][0]  # this loop is bounds_ref's walk
        assert got["samples"][m] <= best + 1e-12 * 12.0 * (N + 1)
    assert exercised > 0  # the policy does exercise at scheduled dates in this case


@pytest.mark.parametrize("N,k", [(1, 2), (7, 7), (12, 15), (13, 13)])
def test_walk_with_the_expiry_alone_gives_q0(N, k):
    So, q, betas = _walk_case(31 * N + k, N)
    got = bs.walk_rows(So, q, range(So.shape[1]), K, R, T, True, betas, k)
    np.testing.assert_allclose(got["samples"], q[:, 0], rtol=0, atol=1e-12 * 12.0)  # Z_N - (Z_N - Q_0)


# ------------------------------------------------------------------ the fuzz cases
def test_fuzz_cases_cover_what_they_promise():
    cases = bs.fuzz_cases(8)
    assert cases == bs.fuzz_cases(8) and cases == bs.fuzz_cases(12)[:8]  # seeded
    assert all(1 <= c["N"] <= 13 and 0 <= c["k"] <= c["N"] + 3 and c["n_inner"] in hc.N_INNER for c in cases)
    assert all(c["n_outer"] % 2 == 0 and 2 <= c["n_outer"] <= 40 and c["n_lower"] % 2 == 0 and c["M"] % 2 == 0 for c in cases)
    assert {c["n_inner"] for c in cases} == set(hc.N_INNER) and len({c["n_outer"] for c in cases}) > 3
    assert 3 * sum(c["refill"] for c in cases) >= len(cases)
    assert {c["model"] for c in cases} == set(bs.MODELS) and {c["is_put"] for c in cases} == {True, False}
    assert {c["policy"] for c in cases} == set(hc.POLICIES)
    assert any(c["policy"] == "given" and any(c["holes"][1:c["N"]]) for c in bs.fuzz_cases(16))
    assert any(c["irr_every"] for c in cases) and not all(c["irr_every"] for c in cases)
    real = [c for c in cases if c["k"] >= 2 and c["J"] >= 2]
    assert len(real) >= 3 and any(c["N"] % c["k"] for c in real)  # schedules with several dates, a short first gap among them
    assert any(c["model"] == "heston1" and not c["feller"] for c in bs.fuzz_cases(16))
    for c in cases:
        p = bs.fuzz_params(c)
        assert (p.n_steps, p.n_paths, p.antithetic) == (c["N"], c["M"], 1)
        assert p.model == _ffi.MODELS["gbm" if c["model"] == "gbm" else "heston"]
        if c["model"] != "gbm":
            assert p.heston_scheme == int(c["model"][-1]) and p.xi == c["xi"]


@pytest.mark.parametrize("case", bs.fuzz_cases(8), ids=lambda c: f"{c['model']}-N{c['N']}-k{c['k']}-i{c['n_inner']}")
def test_fuzz_case_restated_on_numpy_paths(case):
    """Every case on float32 numpy paths: no tie, the scheduled estimators are the all-dates ones of bounds_ref on the holed
    table at the scheduled columns, never more inner steps than the schedule allows, and a never-exercising table takes them all."""
    N, k, n_outer, n_inner = case["N"], case["k"], min(case["n_outer"], 8), min(case["n_inner"], 64)
    is_put = case["is_put"]
    Sl = bs.numpy_paths(case, N + 1, 400, case["S0"], case["seed"])
    So = bs.numpy_paths(case, N + 1, n_outer, case["S0"], case["seed"] + 1)
    inner = lambda i, t: bs.numpy_paths(case, N - t + 1, n_inner, float(So[t, i]), case["seed"] + 7 + i * (N + 1) + t)  # noqa: E731
    rng = np.random.default_rng(case["seed"])
    betas = np.zeros((N + 1, 4))
    betas[1:N, 0], betas[1:N, 1], betas[1:N, 3] = rng.uniform(1.0, 9.0, N - 1), rng.uniform(-30.0, 30.0, N - 1), 40.0
    betas[np.asarray(case["holes"]), 3] = 0.0
    lo = bs.lower_bound(Sl, K, case["r"], case["T"], is_put, betas, k)
    up = bs.upper_bound(So, inner, K, case["r"], case["T"], is_put, betas, k)
    assert lo["ties"] == 0 and up["ties"] == 0
    holed = bs.mask(betas, k)
    taus = bs.schedule(N, k)
    full = br.upper_bound(So, inner, K, case["r"], case["T"], is_put, holed)
    assert np.array_equal(up["q"][:, taus[:-1]], full["q"][:, taus[:-1]])
    off = [t for t in range(N) if t not in taus[:-1]]
    assert np.all(up["q"][:, off] == 0.0)
    assert np.all(up["samples"] <= full["samples"] + br.samples_atol(N, full["q"], full["zmax"]))
    assert lo == br.lower_bound(Sl, K, case["r"], case["T"], is_put, holed)
    assert 0 < up["inner_path_steps"] <= bs.max_inner_steps(N, k, n_outer, n_inner)
    never = bs.upper_bound(So, inner, K, case["r"], case["T"], is_put, np.zeros((N + 1, 4)), k)
    assert never["inner_path_steps"] == bs.max_inner_steps(N, k, n_outer, n_inner)
