"""The refusal table of the eight bounds facades of options_model_amd.api: for each facade a valid call (on device 10^6,
which does not exist) and a list of named keyword sets that each make it invalid -- the sets of the
test_facade(s)_refuse(s)_before_the_device tests, extended until every check of the facade is hit -- taken one at a time
and two at a time.  record() answers, for every such call, which exception comes FIRST: its type and full message, or
REACHED when the call passes every check and asks for its context.  tools/capture_bounds_refusals.py writes the answers to
tests/golden/bounds_facade_refusals.json, tests/test_bounds_facade_refusals_cpu.py replays them."""
import itertools

import numpy as np

from options_model_amd import _ffi, api

REACHED = ["", "reached the context"]  # (type, message) of a call that passed every check
NAN, INF = float("nan"), float("inf")
HP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
ONE = dict(S0=100.0, K=100.0, r=0.05, sigma=0.2, T=1.0, n_paths=1000, n_steps=4, device=10 ** 6)

# what every bounds facade checks: the policy, the given table and the three sizes ...
SIZES = {
    "policy": dict(policy="lattice"), "given-no-betas": dict(policy="given"), "betas-not-given": dict(betas=np.zeros((5, 4))),
    "odd-lower": dict(n_lower=99_999), "odd-outer": dict(n_outer=1023), "odd-inner": dict(n_inner=255),
    "no-inner": dict(n_inner=0),
}
# ... the contract and the path count (sigma: the one-asset facades that take one) ...
CONTRACT = {
    "spot": dict(S0=-100.0), "strike": dict(K=0.0), "expiry": dict(T=0.0), "rate": dict(r=-0.01), "no-paths": dict(n_paths=0),
    "no-steps": dict(n_steps=0), "option-type": dict(option_type="straddle"), "one-path": dict(n_paths=1),
}
SIGMA = {"no-sigma": dict(sigma=None), "negative-sigma": dict(sigma=-0.2)}
# ... and, where it is taken, the schedule
SCHEDULE = {
    "every-none": dict(exercise_every=None), "every-list": dict(exercise_every=[2, 3]), "every-bool": dict(exercise_every=True),
    "every-str": dict(exercise_every="2"), "every-fraction": dict(exercise_every=2.5), "every-negative": dict(exercise_every=-1),
    "every-2^31": dict(exercise_every=2 ** 31),
}
CONTROL = {"cv-2": dict(control_variate=2), "cv-str": dict(control_variate="yes"), "cv-none": dict(control_variate=None),
           "cv-half": dict(control_variate=0.5)}
# the switches of the jump, dividend and barrier laws, and their Heston schemes
SWITCHES = {
    "control-variate": dict(control_variate=True), "european": dict(suboptimality_check="european"),
    "check": dict(suboptimality_check="lattice"), "check-and-schedule": dict(suboptimality_check="payoff", exercise_every=2),
    "model": dict(model="SABR"),
}
SCHEMES = {"calibrator": dict(model="Heston", heston_scheme="calibrator"), "qe": dict(model="Heston", heston_scheme="qe"),
           "scheme": dict(model="Heston", heston_scheme="milstein"), "heston-no-sigma": dict(model="Heston", sigma=None)}
BASKET = dict(spots=[100.0, 95.0], K=100.0, r=0.05, sigmas=[0.2, 0.3], T=1.0, n_paths=1000, n_steps=4, device=10 ** 6)
RUNNERUP = dict(kind="best-of", option_type="call", regressors="index+runner-up")

FACADES = {
    "price_american_bounds": (ONE, {**SCHEDULE, **CONTROL, **SIZES, **CONTRACT, **SIGMA,
                                    "given-short": dict(policy="given", betas=np.zeros((4, 4)))}),
    "price_american_bounds_heston": (
        dict({k: v for k, v in ONE.items() if k != "sigma"}, heston_params=HP),
        {**SCHEDULE, **SIZES, **CONTRACT,
         "sv-schedule": dict(regressors="spot+variance", exercise_every=2),
         "calibrator": dict(heston_scheme="calibrator"), "qe": dict(heston_scheme="qe"), "scheme": dict(heston_scheme="milstein"),
         "regressors": dict(regressors="spot+vol"), "sv-two-pass": dict(regressors="spot+variance", policy="two_pass"),
         "sv-513-steps": dict(regressors="spot+variance", n_steps=513),
         "sv-vbar-zero": dict(regressors="spot+variance", heston_params=dict(HP, v0=0.0, theta=0.0)),
         "betas-cols": dict(policy="given", betas=np.zeros((5, 3))), "betas-rows": dict(policy="given", betas=np.zeros((6, 4))),
         "sv-betas-cols": dict(regressors="spot+variance", policy="given", betas=np.zeros((5, 4)))}),
    "price_american_bounds_jumps": (
        dict(ONE, jump_intensity=1.0, jump_mean=-0.1, jump_vol=0.15),
        {**SWITCHES, **SCHEDULE, **SIZES, **CONTRACT, **SIGMA, **SCHEMES,
         "negative-intensity": dict(jump_intensity=-0.5), "nan-intensity": dict(jump_intensity=NAN),
         "too-intense": dict(jump_intensity=4.5), "negative-vol": dict(jump_vol=-0.1), "infinite-mean": dict(jump_mean=INF),
         "yield": dict(dividend_yield=NAN)}),
    "price_american_bounds_dividends": (
        dict(ONE, dividends=[(0.4, 1.0)]),
        {**SWITCHES, **SCHEDULE, **SIZES, **CONTRACT, **SIGMA, **SCHEMES,
         "yield": dict(dividend_yield=NAN), "item": dict(dividends=[(0.5,)]), "kind": dict(dividends=[(0.5, 1.0, "stock")]),
         "time-0": dict(dividends=[(0.0, 1.0)]), "time-late": dict(dividends=[(1.5, 1.0)]),
         "negative": dict(dividends=[(0.5, -1.0)]), "proportional-1": dict(dividends=[(0.5, 1.0, "proportional")])}),
    "price_barrier_bounds": (
        dict(ONE, barrier=90.0),
        {**SWITCHES, **SCHEDULE, **SIZES, **CONTRACT, **SIGMA, **SCHEMES,
         "continuous": dict(monitoring="continuous"), "barrier-type": dict(barrier_type="down-and-up"),
         "H-0": dict(barrier=0.0), "H-nan": dict(barrier=NAN), "on-the-barrier": dict(barrier=100.0),
         "beyond-down": dict(barrier=101.0), "beyond-up": dict(barrier=99.0, barrier_type="up-and-in"),
         "betas-shape": dict(policy="given", betas=np.zeros((4, 4)))}),
    "price_american_basket_bounds": (
        BASKET,
        {**SIZES, **{k: v for k, v in CONTRACT.items() if k != "spot"},
         "check": dict(suboptimality_check="sometimes"), "european": dict(suboptimality_check="european"),
         "check-and-runner-up": dict(suboptimality_check="payoff", **RUNNERUP),
         "kind": dict(kind="rainbow"), "no-sequence": dict(spots=100.0), "no-assets": dict(spots=[], sigmas=[]),
         "nine-assets": dict(spots=[100.0] * 9, sigmas=[0.2] * 9), "sigmas-short": dict(sigmas=[0.2]),
         "weights-short": dict(weights=[1.0]), "yields-short": dict(dividend_yields=[0.0]),
         "negative-spot": dict(spots=[100.0, -95.0]), "negative-sigma": dict(sigmas=[0.2, -0.3]),
         "negative-weight": dict(weights=[0.5, -0.5]), "nan-yield": dict(dividend_yields=[0.0, NAN]),
         "correlation-shape": dict(correlation=[[1.0]]),
         "regressors": dict(regressors="index+third"), "runner-up-two-pass": dict(RUNNERUP, policy="two_pass"),
         "runner-up-basket": dict(regressors="index+runner-up"),
         "runner-up-one-asset": dict(RUNNERUP, spots=[100.0], sigmas=[0.2]),
         "index+spot-basket": dict(regressors="index+spot"),
         "index+spot-513-steps": dict(regressors="index+spot", kind="asian", n_steps=513),
         "correlation": dict(correlation=[[1.0, 2.0], [2.0, 1.0]]),
         "geometric-correlation": dict(kind="geometric", correlation=[[1.0, 2.0], [2.0, 1.0]])}),
    "price_bermudan_bounds": (
        dict(ONE, exercise_every=2),
        {**SCHEDULE, **CONTROL, "heston-control-variate": dict(model="Heston", control_variate=True),
         "model": dict(model="merton"), "heston": dict(model="Heston"),
         # (handed on to the facade of the model)
         "policy": SIZES["policy"], "odd-inner": SIZES["odd-inner"], "option-type": CONTRACT["option-type"],
         "one-path": CONTRACT["one-path"], "no-sigma": SIGMA["no-sigma"],
         "calibrator": dict(model="Heston", heston_scheme="calibrator"),
         "heston-v0": dict(model="Heston", heston_params=dict(v0="much"))}),
    "price_american_bounds_checked": (
        dict(ONE, check="payoff"),
        {**SCHEDULE, **CONTROL, "check-str": dict(check="yes"), "check-code": dict(check=1), "check-none": dict(check=None),
         "check-case": dict(check="European"), "every-2": dict(exercise_every=2), "every-5": dict(exercise_every=5),
         "model": dict(model="SABR"), "heston": dict(model="Heston"),
         "heston-control-variate": dict(model="Heston", control_variate=True),
         "heston-european": dict(model="Heston", check="european"),
         # (checked by the facade of the model, after the context: never reached here)
         "policy": SIZES["policy"], "option-type": CONTRACT["option-type"]}),
}


class _Reached(Exception):
    pass


def _no_context(device=None):
    assert device == 10 ** 6, device
    raise _Reached


def outcome(facade, kwargs):
    """[type name, message] of the first exception of api.<facade>(**kwargs), REACHED when it is the context's"""
    real = _ffi.default_context
    _ffi.default_context = _no_context
    try:
        getattr(api, facade)(**kwargs)
    except _Reached:
        return list(REACHED)
    except Exception as e:  # whatever comes first is the record
        return [type(e).__name__, str(e)]
    finally:
        _ffi.default_context = real
    raise AssertionError(f"{facade} returned on a device that does not exist")


def calls(facade):
    """(id, keywords) of every call of the table: each set alone, then every unordered pair (the later set's value where
    two sets name one keyword), in the order of FACADES"""
    base, sets = FACADES[facade]
    for a in sets:
        yield a, {**base, **sets[a]}
    for a, b in itertools.combinations(sets, 2):
        yield f"{a} & {b}", {**base, **sets[a], **sets[b]}


def record():
    """{"messages": [[type, message], ...] (each distinct one once), "facades": {name: {"sets": [the names of its sets],
    "first": [index into messages per call of calls(name)]}}}"""
    messages, facades = [], {}
    for facade in FACADES:
        first = []
        for _, kwargs in calls(facade):
            got = outcome(facade, kwargs)
            if got not in messages:
                messages.append(got)
            first.append(messages.index(got))
        facades[facade] = dict(sets=list(FACADES[facade][1]), first=first)
    return dict(messages=messages, facades=facades)
