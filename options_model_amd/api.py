"""North-star facade (BASELINE.json):

    price_american_option(S0, K, r, sigma, T, n_paths, n_steps, model='GBM'|'Heston', ...)

A thin host-side wrapper over the C ABI (include/omc.h).  The reference has no function with
this exact signature; its three real call shapes are mirrored in
`options_model_amd.pricer` (options_model_3.py) and `options_model_amd.compat`
(Options_model.py, options_model_2.py).

semantics (the reference's exercise rule is not textbook LSM, and it is kept):
  "two_pass"  (default) control flow of options_model_3/options_model_3.py:482-651: pass 1
              regresses discounted TERMINAL payoffs with no decisions, pass 2 applies the
              sticky rule; valued at t = dt.  Moments are decision-independent -> one
              all-reduce across GPUs.
  "per_step"  control flow of Options_model.py:108-157 / options_model_2.py:278-313:
              regress-and-decide per time step with the sticky `exercised` mask.
  "textbook"  classic Longstaff-Schwartz (overwrite on earlier exercise, discounted to t=0).
regressor:
  "poly"      OLS on [1,u,u^2], u=S/K-1, one fit per time step (the reference validates
              lsm_poly_degree and then ignores it: Options_model.py:53,69-70)
n_gpus:
  1           this process, one GPU (`device`).
  N > 1       the paths shard by antithetic pair over N GPUs of one node, ONE PROCESS PER GPU; each rank prices its
              shard through the library's own RCCL communicator (dist.RcclPricer: regression moments and result sums
              all-reduced over xGMI) and the call returns the global result.  Two ways to get the ranks:
              * called from a PLAIN process (a script, a notebook, the Streamlit UI -- the reference's callers are
                single-process programs, options_model_2_ui.py:87-133): the ranks are started here as child
                processes on first use (launcher.RankPool: fresh interpreters, the parent never re-execs and makes
                no GPU call for them), keep their communicator across calls and are closed at exit.  `device` may
                list one HIP device per rank (default: rank r -> device r);
              * called by every rank of an N-rank job (`python -m torch.distributed.run --nproc-per-node N
                script.py`, or any launcher that sets RANK / LOCAL_RANK / WORLD_SIZE / MASTER_PORT): each rank is
                its own process already and every rank returns the same global result.
              It never silently prices on fewer GPUs: a rank that cannot start, or a job of another size, raises.
              regressor="nn" shards as well (nn_dist: rows per rank, statistics and gradient partials all-reduced).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field

import numpy as np

from . import _ffi

_SEM = {"two_pass": "two_pass", "v3": "two_pass", "reference_v3": "two_pass",
        "per_step": "reference", "v1": "reference", "reference_v1": "reference",
        "textbook": "textbook"}


@dataclass
class PriceResult:
    price: float
    stderr: float
    std: float
    zero_prob: float
    n_paths: int
    n_exercised: int
    sum_nitm: int
    model: str
    semantics: str
    option_type: str
    timings_ms: dict = field(default_factory=dict)
    info: dict = field(default_factory=dict)  # regressor='nn': trainer, batch, epochs_run, optimizer_steps ...

    def __float__(self):
        return float(self.price)


def _validate(S0, K, T, r, sigma, n_paths, n_steps, option_type, need_sigma=True):
    # same checks and messages as options_model_3.py:447-452,471-472 / Options_model.py:63-72
    if S0 <= 0 or K <= 0 or T <= 0:
        raise ValueError("S0, K, T must be positive.")
    if r < 0:
        raise ValueError("r must be non-negative.")
    if n_paths <= 0 or n_steps <= 0:
        raise ValueError("num_simulations and num_time_steps must be positive integers.")
    if option_type not in ("call", "put"):
        raise ValueError("option_type must be 'call' or 'put'.")
    if need_sigma and (sigma is None or sigma <= 0):
        raise ValueError("sigma is None: provide sigma, iv_model, or heston configuration"
                         if sigma is None else "S0, K, T, and sigma must be positive.")


def _validate_scheme(model_l, heston_scheme, sigma, heston_params):
    """heston_scheme by name or number; "qe" (Andersen's quadratic-exponential rule) needs kappa, theta and xi positive:
    its constants divide by kappa and xi, and the long-run mean is the floor of the next variance's mean."""
    if model_l != "heston":
        return
    if isinstance(heston_scheme, str) and heston_scheme not in _ffi.HESTON_SCHEMES:
        raise ValueError(f"heston_scheme must be one of {sorted(_ffi.HESTON_SCHEMES)}.")
    code = _ffi.HESTON_SCHEMES[heston_scheme] if isinstance(heston_scheme, str) else int(heston_scheme)
    if code == _ffi.HESTON_SCHEMES["qe"]:
        hp = heston_defaults(sigma, heston_params)
        if not (hp["kappa"] > 0 and hp["xi"] > 0 and hp["theta"] > 0):
            raise ValueError("heston_scheme 'qe' needs kappa, theta and xi positive.")


def heston_defaults(sigma, heston_params=None):
    """kappa=2, xi=0.3, rho=-0.7, v0=theta=sigma^2: the reference's hard-coded defaults
    (options_model_3.py:948-950,995-996; options_model_2_ui.py:74-80)."""
    hp = dict(v0=(sigma or 0.2) ** 2, kappa=2.0, theta=(sigma or 0.2) ** 2, xi=0.3, rho=-0.7)
    if heston_params:
        hp.update({k: float(v) for k, v in heston_params.items() if k in hp})
    return hp


def _even_paths(n_paths):
    """n_paths rounded down to whole antithetic pairs (ValueError when none is left)"""
    M = int(n_paths) // 2 * 2
    if M <= 0:
        raise ValueError("num_simulations and num_time_steps must be positive integers.")
    return M


def _dividend_items(dividends):
    """the dividends of a facade -> [(t, amount, kind)]; a bare (t, amount) is a cash dividend (ValueError otherwise)"""
    divs = []
    for d in dividends:
        d = tuple(d)
        if len(d) not in (2, 3):
            raise ValueError("a dividend is (t, amount) or (t, amount, 'cash' | 'proportional').")
        kind = d[2] if len(d) == 3 else "cash"
        if kind not in _ffi.DIVIDEND_KINDS:
            raise ValueError("a dividend's kind must be 'cash' or 'proportional'.")
        divs.append((float(d[0]), float(d[1]), kind))
    return divs


def _jump_args(jump_intensity, jump_mean, jump_vol, dividend_yield):
    """the jump law and the yield of a facade as floats -> (lam, mu, sj, q), each finite (ValueError otherwise)"""
    lam, mu, sj, q = float(jump_intensity), float(jump_mean), float(jump_vol), float(dividend_yield)
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError("jump_intensity must be finite and non-negative.")
    if not math.isfinite(mu):
        raise ValueError("jump_mean must be finite.")
    if not (math.isfinite(sj) and sj >= 0.0):
        raise ValueError("jump_vol must be finite and non-negative.")
    if not math.isfinite(q):
        raise ValueError("dividend_yield must be finite.")
    return lam, mu, sj, q


def price_american_option(S0, K, r, sigma, T, n_paths, n_steps, model="GBM", option_type="put",
                          regressor="poly", semantics="two_pass", heston_params=None,
                          heston_scheme="reference", antithetic=True, seed=42, stream=0,
                          device=None, ctx=None, n_gpus=1, nn_options=None) -> PriceResult:
    """regressor: "poly" (OLS on [1, u, u^2] per time step: the flows of `semantics`), "nn" (the reference's network, two-pass
    flow), "ols7" (one least-squares fit on the reference's 7 features, two-pass flow).
    nn_options (regressor="nn" only): dict with any of nn_hidden, nn_layers, nn_dropout, nn_epochs, nn_lr, nn_batch,
    inference_dropout, torch_seed -- the network named by BASELINE config 5 (2 x 64) by default.
    heston_scheme (model="Heston"): "reference" (= "clamp"), "full_truncation", "calibrator", or "qe" -- Andersen's (2008)
    quadratic-exponential rule, which needs kappa > 0, theta > 0 and xi > 0 (ValueError otherwise)."""
    model_l = str(model).lower()
    n_gpus = int(n_gpus)
    if n_gpus < 1:
        raise ValueError("n_gpus must be a positive integer.")
    if device is None and n_gpus == 1:
        device = _ffi.resolve_device(None)  # 0, or what OMC_DEVICE says ("auto": spread processes over the GPUs)
    if model_l not in ("gbm", "heston"):
        raise ValueError("model must be 'GBM' or 'Heston'.")
    if semantics not in _SEM:
        raise ValueError(f"semantics must be one of {sorted(set(_SEM))}.")
    if regressor not in ("poly", "nn", "ols7"):
        raise ValueError("regressor must be 'poly', 'nn' or 'ols7'.")
    if n_gpus > 1 and not _in_job(n_gpus):
        # a plain process: validate here (the reference's messages), then let the rank pool do the collective call
        if ctx is not None:
            raise ValueError("n_gpus > 1 uses one context per rank process; do not pass ctx.")
        _validate(S0, K, T, r, sigma, n_paths, n_steps, option_type, need_sigma=(model_l == "gbm"))
        _validate_scheme(model_l, heston_scheme, sigma, heston_params)
        from . import launcher
        if isinstance(device, int) and not os.environ.get("OMC_RCCL_LIB"):
            # (real RCCL refuses two ranks on one card; only the shared-memory stand-in of the tests runs that way)
            raise ValueError("n_gpus > 1 needs one device per rank: pass device=[d0, d1, ...] or leave it unset.")
        devices = None if device is None else ([int(device)] * n_gpus if isinstance(device, int) else list(device))
        if devices is not None and len(devices) != n_gpus:
            raise ValueError(f"device lists {len(devices)} cards for n_gpus={n_gpus}.")
        kw = dict(S0=S0, K=K, r=r, sigma=sigma, T=T, n_paths=int(n_paths), n_steps=int(n_steps), model=model,
                  option_type=option_type, heston_params=heston_params, seed=int(seed), stream=int(stream))
        if regressor == "nn":
            kw.update(nn_options or {})
            d = launcher.pool(n_gpus, devices).call("price_american_option_nn", kw, timeout_s=3600.0)
        else:
            kw.update(regressor=regressor, semantics=semantics, heston_scheme=heston_scheme, antithetic=bool(antithetic))
            d = launcher.pool(n_gpus, devices).call("price_american_option", kw)
        d["info"] = dict(d.get("info", {}), launched_ranks=n_gpus)
        return PriceResult(**d)
    if regressor == "ols7":
        # ONE global least-squares fit on the reference's seven features (options_model_3.py:105-121) in its two-pass flow
        # (omc_price_american_ols7): the linear regressor between the per-step polynomial and the network.  Across GPUs the
        # paths shard by antithetic pair and the ranks' co-moments are merged by two small all-reduces: the fit is the job's.
        _validate(S0, K, T, r, sigma, n_paths, n_steps, option_type, need_sigma=(model_l == "gbm"))
        _validate_scheme(model_l, heston_scheme, sigma, heston_params)
        M = int(n_paths) // 2 * 2 if antithetic else int(n_paths)
        if M <= 0:
            raise ValueError("num_simulations and num_time_steps must be positive integers.")
        kwp = dict(model=model_l, is_put=(option_type == "put"), semantics="two_pass", antithetic=antithetic,
                   heston_scheme=heston_scheme, n_steps=int(n_steps), S0=S0, K=K, r=r, sigma=sigma or 0.0, T=T, seed=seed,
                   stream=stream, **heston_defaults(sigma, heston_params))
        info = dict(regressor="ols7")
        if n_gpus > 1:
            if ctx is not None:
                raise ValueError("n_gpus > 1 uses the job's own per-rank context; do not pass ctx.")
            sp = _job_pricer(n_gpus, device)
            out = sp.price_american_ols7(M, **kwp)
            info.update(n_gpus=n_gpus, rank=sp.rank, transport=sp.transport)
        else:
            c = ctx or _ffi.default_context(_ffi.resolve_device(None) if device is None else device)
            out = c.price_american_ols7(_ffi.make_params(n_paths=M, **kwp))
        Mg = out["n_paths"]
        var = max(out["sumsq"] / Mg - out["price"] ** 2, 0.0)
        info.update(weights=[float(v) for v in out["weights"]], y_mean=out["y_mean"], y_std=out["y_std"])
        return PriceResult(price=out["price"], stderr=math.sqrt(var / Mg), std=out["std"], zero_prob=out["zero_prob"], n_paths=Mg,
                           n_exercised=out["n_exercised"], sum_nitm=out["sum_nitm"], model=model_l, semantics="two_pass",
                           option_type=option_type, info=info)
    if regressor == "nn":
        if n_gpus > 1:
            from . import nn_dist
            return nn_dist.price_american_option_nn_sharded(
                _job_pricer(n_gpus, device), S0, K, r, sigma, T, n_paths, n_steps, model=model,
                option_type=option_type, heston_params=heston_params, seed=seed, stream=stream, **(nn_options or {}))
        from . import nn_regressor
        return nn_regressor.price_american_option_nn(
            S0, K, r, sigma, T, n_paths, n_steps, model=model, option_type=option_type,
            heston_params=heston_params, seed=seed, stream=stream, device=device, **(nn_options or {}))
    _validate(S0, K, T, r, sigma, n_paths, n_steps, option_type, need_sigma=(model_l == "gbm"))
    _validate_scheme(model_l, heston_scheme, sigma, heston_params)
    M = int(n_paths) // 2 * 2 if antithetic else int(n_paths)  # options_model_3.py:458
    if M <= 0:
        raise ValueError("num_simulations and num_time_steps must be positive integers.")
    hp = heston_defaults(sigma, heston_params)
    if n_gpus > 1:
        if ctx is not None:
            raise ValueError("n_gpus > 1 uses the job's own per-rank context; do not pass ctx.")
        sp = _job_pricer(n_gpus, device)
        out = sp.price_american(M, model=model_l, is_put=(option_type == "put"), semantics=_SEM[semantics],
                                antithetic=antithetic, heston_scheme=heston_scheme, n_steps=int(n_steps), S0=S0,
                                K=K, r=r, sigma=sigma or 0.0, T=T, seed=seed, stream=stream, **hp)
        loc = out["local"]
        return PriceResult(price=out["price"], stderr=out["stderr"], std=out["std"], zero_prob=out["zero_prob"],
                           n_paths=out["n_paths"], n_exercised=out["n_exercised"], sum_nitm=out["sum_nitm"],
                           model=model_l, semantics=semantics, option_type=option_type,
                           timings_ms=dict(paths=loc["ms_paths"], lsm=loc["ms_lsm"], total=loc["ms_total"]),
                           info=dict(n_gpus=n_gpus, rank=sp.rank, transport=sp.transport))
    c = ctx or _ffi.default_context(device)
    p = _ffi.make_params(model=model_l, is_put=(option_type == "put"), semantics=_SEM[semantics],
                         antithetic=antithetic, heston_scheme=heston_scheme, n_paths=M,
                         n_steps=int(n_steps), S0=S0, K=K, r=r, sigma=sigma or 0.0, T=T,
                         seed=seed, stream=stream, **hp)
    out = c.price_american(p)
    var = max(out["sumsq"] / M - out["price"] ** 2, 0.0)
    return PriceResult(price=out["price"], stderr=math.sqrt(var / M), std=out["std"],
                       zero_prob=out["zero_prob"], n_paths=M, n_exercised=out["n_exercised"],
                       sum_nitm=out["sum_nitm"], model=model_l, semantics=semantics,
                       option_type=option_type,
                       timings_ms=dict(paths=out["ms_paths"], lsm=out["ms_lsm"], total=out["ms_total"]))


def exercise_dates(n_steps, exercise_every):
    """The early-exercise dates of a schedule on a grid of n_steps dates (omc_chain_entry::exercise_every): every date
    1 .. n_steps-1 for 0 or 1, else the dates t with (n_steps - t) % exercise_every == 0 -- every k-th date counted back
    from expiry, which is no early date itself."""
    N, k = int(n_steps), int(exercise_every)
    if k < 0:
        raise ValueError("exercise_every must be a non-negative integer.")
    return [t for t in range(1, N) if k < 2 or (N - t) % k == 0]


def _one_schedule(k):
    """one exercise_every -> a non-negative int (ValueError otherwise)"""
    if isinstance(k, bool) or not isinstance(k, (int, float)) and not hasattr(k, "__index__"):
        raise ValueError("exercise_every must be a non-negative integer.")
    if isinstance(k, float) and not (math.isfinite(k) and k == int(k)):
        raise ValueError("exercise_every must be a non-negative integer.")
    k = int(k)
    if k < 0 or k > 2 ** 31 - 1:
        raise ValueError("exercise_every must be a non-negative integer.")
    return k


def bounds_exercise_dates(n_steps, exercise_every):
    """The exercise dates of the price bounds' game on a grid of n_steps dates (option "bounds_exercise_every"): every date
    1 .. n_steps for 0 or 1, else the dates of exercise_dates -- every k-th date counted back from expiry -- and the expiry
    itself: (n_steps - 1) // k + 1 dates."""
    N, k = int(n_steps), _one_schedule(exercise_every)
    return [t for t in range(1, N + 1) if k < 2 or (N - t) % k == 0]


def _schedules(exercise_every, n):
    """exercise_every of price_american_chain -> one non-negative int per strike (ValueError otherwise)."""
    one = _one_schedule
    if exercise_every is None:
        return [0] * n
    if isinstance(exercise_every, (str, bytes)):
        raise ValueError("exercise_every must be a non-negative integer.")
    try:
        ks = list(exercise_every)
    except TypeError:
        return [one(exercise_every)] * n
    if len(ks) != n:
        raise ValueError("exercise_every must be one integer or one per strike.")
    return [one(k) for k in ks]


@dataclass
class ChainResult:
    """price_american_chain: one PriceResult per quote, filled as price_american_option fills it; its info carries the
    quote's schedule (exercise_every, n_early_dates)."""
    entries: list
    strikes: list
    option_types: list
    exercise_every: list = field(default_factory=list)  # per quote: 0 = every date
    timings_ms: dict = field(default_factory=dict)  # whole chain: paths, pass1, pass2, total
    info: dict = field(default_factory=dict)        # folded, fused, n_launch_groups

    def __len__(self):
        return len(self.entries)

    def __getitem__(self, i):
        return self.entries[i]


def _chain_checked(S0, strikes, r, sigma, T, n_paths, n_steps, option_types, model, heston_params, heston_scheme,
                   exercise_every, n_gpus):
    """price_american_chain's argument checks, in its order -> (model, strikes, sides, schedules, paths); ValueError otherwise"""
    model_l = str(model).lower()
    if model_l not in ("gbm", "heston"):
        raise ValueError("model must be 'GBM' or 'Heston'.")
    if isinstance(n_gpus, bool) or n_gpus != 1:
        raise ValueError("a chain is priced on one GPU (n_gpus = 1).")
    try:
        ks = [float(k) for k in strikes]
    except TypeError:
        raise ValueError("strikes must be a sequence of numbers.") from None
    if not ks:
        raise ValueError("strikes must not be empty.")
    if len(ks) > _ffi.CHAIN_MAX:
        raise ValueError(f"a chain has at most {_ffi.CHAIN_MAX} entries.")
    types = [option_types] * len(ks) if isinstance(option_types, str) else list(option_types)
    if len(types) != len(ks):
        raise ValueError("option_types must be one string or one per strike.")
    every = _schedules(exercise_every, len(ks))
    for k, ot in zip(ks, types):
        if not (math.isfinite(k) and k > 0):
            raise ValueError("S0, K, T must be positive.")
        _validate(S0, k, T, r, sigma, n_paths, n_steps, ot, need_sigma=(model_l == "gbm"))
        _validate_scheme(model_l, heston_scheme, sigma, heston_params)
    return model_l, ks, types, every, _even_paths(n_paths)


def price_american_chain(S0, strikes, r, sigma, T, n_paths, n_steps, option_types="put", model="GBM", heston_params=None,
                         heston_scheme="reference", seed=42, stream=0, device=None, ctx=None, exercise_every=None,
                         n_gpus=1) -> ChainResult:
    """Every quote of one expiry -- `strikes`, each a put or a call (`option_types`: one string for all, or one per
    strike) -- from ONE set of paths (omc_price_american_chain): two-pass flow, polynomial regressor, antithetic pairs,
    one GPU.  entries[i] equals price_american_option(S0, strikes[i], ..., option_type=option_types[i]) bit for bit.
    exercise_every: None (every quote American), one int for all quotes or one per strike -- 0 or 1 every date, k >= 2 a
    Bermudan quote that may exercise early only at every k-th date counted back from expiry (exercise_dates); the
    American, Bermudan and European (k >= n_steps) values of a strike then come from the same paths.
    heston_scheme (model="Heston"): "reference" (= "clamp"), "full_truncation", "calibrator", or "qe" -- Andersen's (2008)
    quadratic-exponential rule, which needs kappa > 0, theta > 0 and xi > 0 (ValueError otherwise)."""
    model_l, ks, types, every, M = _chain_checked(S0, strikes, r, sigma, T, n_paths, n_steps, option_types, model,
                                                  heston_params, heston_scheme, exercise_every, n_gpus)
    c = ctx or _ffi.default_context(device)
    p = _ffi.make_params(model=model_l, is_put=True, semantics="two_pass", antithetic=True, heston_scheme=heston_scheme,
                         n_paths=M, n_steps=int(n_steps), S0=S0, K=ks[0], r=r, sigma=sigma or 0.0, T=T, seed=seed,
                         stream=stream, **heston_defaults(sigma, heston_params))
    outs, info = c.price_american_chain(p, ks, [ot == "put" for ot in types], exercise_every=every)
    entries = []
    for out, ot, k in zip(outs, types, every):
        var = max(out["sumsq"] / M - out["price"] ** 2, 0.0)
        entries.append(PriceResult(price=out["price"], stderr=math.sqrt(var / M), std=out["std"],
                                   zero_prob=out["zero_prob"], n_paths=M, n_exercised=out["n_exercised"],
                                   sum_nitm=out["sum_nitm"], model=model_l, semantics="two_pass", option_type=ot,
                                   timings_ms=dict(paths=out["ms_paths"], lsm=out["ms_lsm"], total=out["ms_total"]),
                                   info=dict(exercise_every=k, n_early_dates=len(exercise_dates(n_steps, k)))))
    return ChainResult(entries=entries, strikes=ks, option_types=types, exercise_every=every,
                       timings_ms=dict(paths=info["ms_paths"], pass1=info["ms_pass1"], pass2=info["ms_pass2"],
                                       total=info["ms_total"]),
                       info=dict(folded=bool(info["folded"]), fused=bool(info["fused"]),
                                 n_launch_groups=info["n_launch_groups"]))


def price_bermudan_option(S0, K, r, sigma, T, n_paths, n_steps, exercise_every, model="GBM", option_type="put",
                          heston_params=None, heston_scheme="reference", seed=42, stream=0, device=None,
                          ctx=None) -> PriceResult:
    """A Bermudan option on a grid of n_steps dates that may be exercised early at every exercise_every-th date counted
    back from expiry (exercise_dates): the one-entry chain (price_american_chain), two-pass flow, polynomial regressor,
    antithetic pairs, one GPU.  0 or 1 is the American option, exercise_every >= n_steps the European value of the flow.
    The result is price_american_option's; info carries exercise_every, n_early_dates and the storage."""
    if exercise_every is None or isinstance(exercise_every, (list, tuple)):
        raise ValueError("exercise_every must be a non-negative integer.")
    chain = price_american_chain(S0, [K], r, sigma, T, n_paths, n_steps, option_types=option_type, model=model,
                                 heston_params=heston_params, heston_scheme=heston_scheme, seed=seed, stream=stream,
                                 device=device, ctx=ctx, exercise_every=exercise_every)
    out = chain.entries[0]
    out.info = dict(out.info, folded=chain.info["folded"])
    return out


@dataclass
class GreeksResult:
    """price_american_greeks: the frozen-policy pathwise Greeks of the two-pass poly estimator, in raw units (per unit
    S0, S0^2, sigma, r; theta = -dV/dT per year).  Heston: vega, rho, theta are NaN."""
    price: float
    stderr: float
    delta: float
    gamma: float
    vega: float
    rho: float
    theta: float
    se_delta: float
    se_gamma: float
    se_vega: float
    se_rho: float
    se_theta: float
    price_up: float
    price_down: float
    bump: float
    n_paths: int
    n_exercised: int
    folded: bool
    model: str
    option_type: str
    timings_ms: dict = field(default_factory=dict)

    def as_reference_dict(self) -> dict:
        """The keys and units of the reference's BlackScholesGreeks.greeks: Vega and Rho per 1 %, Theta per day."""
        return {"Delta": self.delta, "Gamma": self.gamma, "Vega": self.vega / 100, "Theta": self.theta / 365,
                "Rho": self.rho / 100}


def price_american_greeks(S0, K, r, sigma, T, n_paths, n_steps, model="GBM", option_type="put", heston_params=None,
                          heston_scheme="reference", antithetic=True, seed=42, stream=0, device=None, ctx=None,
                          n_gpus=1, bump=0.01) -> GreeksResult:
    """Delta, gamma, vega, rho and theta of the American price of price_american_option(regressor="poly",
    semantics="two_pass") with the exercise policy pass 1 fits held fixed (omc_price_american_greeks).  They are exact
    derivatives of that frozen-policy estimator; they differ from the true American Greeks only through the policy's
    suboptimality.  gamma is a central difference of pathwise deltas at S0 (1 +- bump) on the same paths.  One GPU.
    heston_scheme (model="Heston"): "reference" (= "clamp"), "full_truncation", "calibrator", or "qe" -- Andersen's (2008)
    quadratic-exponential rule, which needs kappa > 0, theta > 0 and xi > 0 (ValueError otherwise).  The spot of every
    scheme is linear in S0, so the Heston delta and gamma need nothing of the scheme."""
    model_l = str(model).lower()
    if int(n_gpus) != 1:
        raise ValueError("price_american_greeks runs on one GPU (n_gpus=1).")
    if model_l not in ("gbm", "heston"):
        raise ValueError("model must be 'GBM' or 'Heston'.")
    if not (0.0 < float(bump) <= 0.5):
        raise ValueError("bump must lie in (0, 0.5].")
    _validate(S0, K, T, r, sigma, n_paths, n_steps, option_type, need_sigma=(model_l == "gbm"))
    _validate_scheme(model_l, heston_scheme, sigma, heston_params)
    M = int(n_paths) // 2 * 2 if antithetic else int(n_paths)
    if M <= 0:
        raise ValueError("num_simulations and num_time_steps must be positive integers.")
    c = ctx or _ffi.default_context(device)
    p = _ffi.make_params(model=model_l, is_put=(option_type == "put"), semantics="two_pass", antithetic=antithetic,
                         heston_scheme=heston_scheme, n_paths=M, n_steps=int(n_steps), S0=S0, K=K, r=r,
                         sigma=sigma or 0.0, T=T, seed=seed, stream=stream, **heston_defaults(sigma, heston_params))
    out = c.price_american_greeks(p, bump=float(bump))
    var = max(out["sumsq"] / M - out["price"] ** 2, 0.0)
    return GreeksResult(price=out["price"], stderr=math.sqrt(var / M), delta=out["delta"], gamma=out["gamma"],
                        vega=out["vega"], rho=out["rho"], theta=out["theta"], se_delta=out["se_delta"],
                        se_gamma=out["se_gamma"], se_vega=out["se_vega"], se_rho=out["se_rho"], se_theta=out["se_theta"],
                        price_up=out["price_up"], price_down=out["price_down"], bump=out["bump"], n_paths=M,
                        n_exercised=out["n_exercised"], folded=bool(out["folded"]), model=model_l,
                        option_type=option_type,
                        timings_ms=dict(paths=out["ms_paths"], pass1=out["ms_pass1"], greeks=out["ms_greeks"],
                                        total=out["ms_total"]))


@dataclass
class ChainGreeksResult:
    """price_american_chain_greeks: one GreeksResult per quote, in the caller's order, the quotes' schedules (entry_info[i]:
    exercise_every, n_early_dates, sum_nitm) and what the chain as a whole did."""
    entries: list
    strikes: list
    option_types: list
    exercise_every: list = field(default_factory=list)  # per quote: 0 = every date
    entry_info: list = field(default_factory=list)      # per quote: dict(exercise_every, n_early_dates, sum_nitm)
    timings_ms: dict = field(default_factory=dict)  # whole chain: paths, pass1, greeks, total
    info: dict = field(default_factory=dict)        # folded, n_groups, n_sweep_launches, entries_per_launch

    def __len__(self):
        return len(self.entries)

    def __getitem__(self, i):
        return self.entries[i]


def price_american_chain_greeks(S0, strikes, r, sigma, T, n_paths, n_steps, option_types="put", exercise_every=None,
                                model="GBM", heston_params=None, heston_scheme="reference", bump=0.01, betas=None, seed=42,
                                stream=0, device=None, ctx=None) -> ChainGreeksResult:
    """Delta, gamma, vega, rho and theta of every quote of one expiry -- `strikes`, sides (`option_types`) and schedules
    (`exercise_every`) as price_american_chain takes them -- from ONE set of paths (omc_price_american_chain_greeks, DESIGN.md
    section 35).  An American entry equals price_american_greeks(S0, strikes[i], ..., option_type=option_types[i]) bit for
    bit; a Bermudan entry (exercise_every >= 2) is the frozen-policy estimator of price_bermudan_option: the American,
    Bermudan and European (k >= n_steps) hedges of a strike then come from the same paths.  betas: None, or one given policy
    per quote, [len(strikes)][n_steps+1][4].  Heston: vega, rho, theta are NaN.  One GPU."""
    model_l, ks, types, every, M = _chain_checked(S0, strikes, r, sigma, T, n_paths, n_steps, option_types, model,
                                                  heston_params, heston_scheme, exercise_every, 1)
    if not (0.0 < float(bump) <= 0.5):
        raise ValueError("bump must lie in (0, 0.5].")
    if betas is not None and np.shape(betas) != (len(ks), int(n_steps) + 1, 4):
        raise ValueError(f"betas must have shape ({len(ks)}, {int(n_steps) + 1}, 4), got {np.shape(betas)}.")
    c = ctx or _ffi.default_context(device)
    p = _ffi.make_params(model=model_l, is_put=True, semantics="two_pass", antithetic=True, heston_scheme=heston_scheme,
                         n_paths=M, n_steps=int(n_steps), S0=S0, K=ks[0], r=r, sigma=sigma or 0.0, T=T, seed=seed,
                         stream=stream, **heston_defaults(sigma, heston_params))
    outs, info = c.price_american_chain_greeks(p, ks, [ot == "put" for ot in types], bump=float(bump), betas=betas,
                                               exercise_every=every)
    entries, entry_info = [], []
    for out, ot, k in zip(outs, types, every):
        var = max(out["sumsq"] / M - out["price"] ** 2, 0.0)
        g = GreeksResult(price=out["price"], stderr=math.sqrt(var / M), delta=out["delta"], gamma=out["gamma"],
                         vega=out["vega"], rho=out["rho"], theta=out["theta"], se_delta=out["se_delta"],
                         se_gamma=out["se_gamma"], se_vega=out["se_vega"], se_rho=out["se_rho"], se_theta=out["se_theta"],
                         price_up=out["price_up"], price_down=out["price_down"], bump=out["bump"], n_paths=M,
                         n_exercised=out["n_exercised"], folded=bool(out["folded"]), model=model_l, option_type=ot,
                         timings_ms=dict(paths=out["ms_paths"], pass1=out["ms_pass1"], greeks=out["ms_greeks"],
                                         total=out["ms_total"]))
        entries.append(g)
        entry_info.append(dict(exercise_every=k, n_early_dates=len(exercise_dates(n_steps, k)), sum_nitm=out["sum_nitm"]))
    return ChainGreeksResult(entries=entries, strikes=ks, option_types=types, exercise_every=every, entry_info=entry_info,
                             timings_ms=dict(paths=info["ms_paths"], pass1=info["ms_pass1"], greeks=info["ms_greeks"],
                                             total=info["ms_total"]),
                             info=dict(folded=bool(info["folded"]), n_groups=info["n_groups"],
                                       n_sweep_launches=info["n_sweep_launches"],
                                       entries_per_launch=info["entries_per_launch"]))


def price_bermudan_greeks(S0, K, r, sigma, T, n_paths, n_steps, exercise_every, model="GBM", option_type="put",
                          heston_params=None, heston_scheme="reference", bump=0.01, seed=42, stream=0, device=None,
                          ctx=None) -> GreeksResult:
    """The frozen-policy pathwise Greeks of the Bermudan option of price_bermudan_option: the one-entry chain
    (price_american_chain_greeks).  0 or 1 is the American option (price_american_greeks' bits), exercise_every >= n_steps
    the European Greeks of the flow."""
    if exercise_every is None or isinstance(exercise_every, (list, tuple)):
        raise ValueError("exercise_every must be a non-negative integer.")
    chain = price_american_chain_greeks(S0, [K], r, sigma, T, n_paths, n_steps, option_types=option_type,
                                        exercise_every=exercise_every, model=model, heston_params=heston_params,
                                        heston_scheme=heston_scheme, bump=bump, seed=seed, stream=stream, device=device,
                                        ctx=ctx)
    return chain.entries[0]


@dataclass
class BarrierResult:
    """price_barrier_option: price / stderr of the option of `barrier_type` in the asked style, the European knock-out
    and knock-in on the same paths (euro_in + euro_out = the vanilla European, path by path) and the hit probability."""
    price: float
    stderr: float
    n_exercised: int
    hit_prob: float
    euro_out: float
    euro_out_se: float
    euro_in: float
    euro_in_se: float
    n_paths: int
    barrier: float
    barrier_type: str
    option_type: str
    style: str
    monitoring: str
    model: str
    timings_ms: dict = field(default_factory=dict)

    def __float__(self):
        return float(self.price)


def price_barrier_option(S0, K, r, sigma, T, n_paths, n_steps, barrier, barrier_type="down-and-out", option_type="put",
                         style="american", monitoring="discrete", model="GBM", heston_params=None,
                         heston_scheme="reference", seed=42, stream=0, device=None, ctx=None) -> BarrierResult:
    """Knock-in / knock-out barrier option (omc_price_barrier).  style "american": the two-pass poly
    LSM (price_american_option(semantics="two_pass")) on the path matrix with the spots where the option is not live
    replaced by a dead spot; "european": the discounted terminal payoff, no matrix.  monitoring "discrete" (grid steps
    1..n_steps) or "continuous" (GBM: Brownian-bridge crossing test between grid points).  Antithetic paths, one GPU.
    heston_scheme (model="Heston"): "reference" (= "clamp"), "full_truncation", "calibrator", or "qe" -- Andersen's (2008)
    quadratic-exponential rule, which needs kappa > 0, theta > 0 and xi > 0 (ValueError otherwise)."""
    model_l = str(model).lower()
    if model_l not in ("gbm", "heston"):
        raise ValueError("model must be 'GBM' or 'Heston'.")
    if barrier_type not in _ffi.BARRIER_KINDS:
        raise ValueError(f"barrier_type must be one of {sorted(_ffi.BARRIER_KINDS)}.")
    if style not in ("american", "european"):
        raise ValueError("style must be 'american' or 'european'.")
    if monitoring not in _ffi.MONITORING:
        raise ValueError("monitoring must be 'discrete' or 'continuous'.")
    if monitoring == "continuous" and model_l != "gbm":
        raise ValueError("continuous barrier monitoring is available for GBM only.")
    if not (math.isfinite(float(barrier)) and float(barrier) > 0):
        raise ValueError("barrier H must be finite and positive.")
    _validate(S0, K, T, r, sigma, n_paths, n_steps, option_type, need_sigma=(model_l == "gbm"))
    _validate_scheme(model_l, heston_scheme, sigma, heston_params)
    M = _even_paths(n_paths)
    c = ctx or _ffi.default_context(device)
    p = _ffi.make_params(model=model_l, is_put=(option_type == "put"), semantics="two_pass", antithetic=True,
                         heston_scheme=heston_scheme, n_paths=M, n_steps=int(n_steps), S0=S0, K=K, r=r,
                         sigma=sigma or 0.0, T=T, seed=seed, stream=stream, **heston_defaults(sigma, heston_params))
    out = c.price_barrier(p, barrier_type, float(barrier), monitoring=monitoring, american=(style == "american"))
    var = max(out["sumsq"] / M - out["price"] ** 2, 0.0)
    timings = dict(barrier_paths=out["ms_barrier_paths"], total=out["ms_total"])
    if style == "american":
        timings.update(pass1=out["ms_pass1"], pass2=out["ms_pass2"], lsm=out["ms_lsm"])
    return BarrierResult(price=out["price"], stderr=math.sqrt(var / M), n_exercised=out["n_exercised"],
                         hit_prob=out["hit_prob"], euro_out=out["euro_out"], euro_out_se=out["euro_out_se"],
                         euro_in=out["euro_in"], euro_in_se=out["euro_in_se"], n_paths=M, barrier=float(barrier),
                         barrier_type=barrier_type, option_type=option_type, style=style, monitoring=monitoring,
                         model=model_l, timings_ms=timings)


@dataclass
class DividendResult:
    """price_american_dividends: price / stderr (the convention of PriceResult), the exercise counts, the storage the
    pricing ran on and the time steps on which a dividend went ex."""
    price: float
    stderr: float
    std: float
    zero_prob: float
    n_paths: int
    n_exercised: int
    sum_nitm: int
    folded: bool
    dividend_steps: int
    dividend_yield: float
    model: str
    option_type: str
    timings_ms: dict = field(default_factory=dict)
    info: dict = field(default_factory=dict)  # first_dividend_step, n_dividends

    def __float__(self):
        return float(self.price)


def price_american_dividends(S0, K, r, sigma, T, n_paths, n_steps, dividend_yield=0.0, dividends=(), model="GBM",
                             option_type="put", heston_params=None, seed=42, device=None,
                             heston_scheme="reference") -> DividendResult:
    """American option on a stock that pays dividends (omc_price_american_div): the two-pass poly
    LSM of price_american_option on paths that drift at r - dividend_yield and drop by every discrete dividend on its
    ex-dividend step.  dividends: items (t, amount) -- a cash dividend -- or (t, amount, "cash" | "proportional"), with
    0 < t <= T; a proportional amount is the fraction of the spot paid out, in [0, 1).  Antithetic paths, one GPU.
    heston_scheme (model="Heston"): "reference" (= "clamp"), "full_truncation", "calibrator", or "qe" -- Andersen's (2008)
    quadratic-exponential rule, which needs kappa > 0, theta > 0 and xi > 0 (ValueError otherwise)."""
    model_l = str(model).lower()
    if model_l not in ("gbm", "heston"):
        raise ValueError("model must be 'GBM' or 'Heston'.")
    q = float(dividend_yield)
    if not math.isfinite(q):
        raise ValueError("dividend_yield must be finite.")
    divs = _dividend_items(dividends)
    _validate(S0, K, T, r, sigma, n_paths, n_steps, option_type, need_sigma=(model_l == "gbm"))
    _validate_scheme(model_l, heston_scheme, sigma, heston_params)
    M = _even_paths(n_paths)
    c = _ffi.default_context(device)
    p = _ffi.make_params(model=model_l, is_put=(option_type == "put"), semantics="two_pass", antithetic=True,
                         n_paths=M, n_steps=int(n_steps), S0=S0, K=K, r=r, sigma=sigma or 0.0, T=T, seed=seed,
                         heston_scheme=heston_scheme, **heston_defaults(sigma, heston_params))
    out = c.price_american_div(p, q, divs)
    var = max(out["sumsq"] / M - out["price"] ** 2, 0.0)
    return DividendResult(price=out["price"], stderr=math.sqrt(var / M), std=out["std"], zero_prob=out["zero_prob"],
                          n_paths=M, n_exercised=out["n_exercised"], sum_nitm=out["sum_nitm"],
                          folded=bool(out["folded"]), dividend_steps=out["n_div_steps"], dividend_yield=q, model=model_l,
                          option_type=option_type,
                          timings_ms=dict(paths=out["ms_div_paths"], pass1=out["ms_pass1"], pass2=out["ms_pass2"],
                                          lsm=out["ms_lsm"], total=out["ms_total"]),
                          info=dict(first_dividend_step=out["first_div_step"], n_dividends=len(divs)))


@dataclass
class DividendGreeksResult:
    """price_american_dividend_greeks: the frozen-policy price and its pathwise Greeks in raw units (per unit S0 / S0^2 /
    sigma / r / q / year), their standard errors, the bumped scenarios and the policy used.  Heston: vega, rho, theta and
    epsilon are NaN."""
    price: float
    stderr: float
    delta: float
    gamma: float
    vega: float
    rho: float
    theta: float
    epsilon: float
    se_delta: float
    se_gamma: float
    se_vega: float
    se_rho: float
    se_theta: float
    se_epsilon: float
    price_up: float
    price_down: float
    bump: float
    n_paths: int
    n_exercised: int
    n_exercised_up: int
    n_exercised_down: int
    sum_nitm: int
    folded: bool
    dividend_steps: int
    first_dividend_step: int
    dividend_yield: float
    model: str
    option_type: str
    betas: object = None  # numpy [n_steps+1][4]: b0, b1, b2, n
    timings_ms: dict = field(default_factory=dict)

    def __float__(self):
        return float(self.price)


def price_american_dividend_greeks(S0, K, r, sigma, T, n_paths, n_steps, dividend_yield=0.0, dividends=(), model="GBM",
                                   option_type="put", heston_params=None, heston_scheme="reference", seed=42, stream=0,
                                   bump=0.01, betas=None, device=None, ctx=None) -> DividendGreeksResult:
    """Delta, gamma, vega, rho, theta and epsilon (dV/d dividend_yield) of the American price price_american_dividends
    quotes, with the exercise policy pass 1 fits -- or `betas` [n_steps+1][4] -- held fixed (omc_price_american_div_greeks,
    DESIGN.md section 32).  One forward sweep regenerates the paths and carries their tangents through every dividend: a
    cash dividend makes the spot affine in S0, which price_american_greeks' scaled paths cannot follow.  theta is -dV/dT at
    fixed n_steps with the dividends fixed on their steps and at their amounts; there is no sensitivity to a dividend's
    amount.  Heston gives delta and gamma; the others are NaN.  dividends and heston_scheme: as price_american_dividends
    takes them.  Antithetic paths, one GPU."""
    model_l = str(model).lower()
    if model_l not in ("gbm", "heston"):
        raise ValueError("model must be 'GBM' or 'Heston'.")
    q = float(dividend_yield)
    if not math.isfinite(q):
        raise ValueError("dividend_yield must be finite.")
    if not (0.0 < float(bump) <= 0.5):
        raise ValueError("bump must lie in (0, 0.5].")
    divs = _dividend_items(dividends)
    _validate(S0, K, T, r, sigma, n_paths, n_steps, option_type, need_sigma=(model_l == "gbm"))
    _validate_scheme(model_l, heston_scheme, sigma, heston_params)
    M = _even_paths(n_paths)
    p = _ffi.make_params(model=model_l, is_put=(option_type == "put"), semantics="two_pass", antithetic=True,
                         n_paths=M, n_steps=int(n_steps), S0=S0, K=K, r=r, sigma=sigma or 0.0, T=T, seed=seed,
                         stream=stream, heston_scheme=heston_scheme, **heston_defaults(sigma, heston_params))
    _ffi.dividend_schedule(p, q, divs)  # (host only: the library's own checks of the schedule, before a context)
    c = ctx or _ffi.default_context(device)
    out = c.price_american_dividend_greeks(p, q, divs, bump=float(bump), betas=betas, want_betas=True)
    var = max(out["sumsq"] / M - out["price"] ** 2, 0.0)
    return DividendGreeksResult(
        price=out["price"], stderr=math.sqrt(var / M), delta=out["delta"], gamma=out["gamma"], vega=out["vega"],
        rho=out["rho"], theta=out["theta"], epsilon=out["epsilon"], se_delta=out["se_delta"], se_gamma=out["se_gamma"],
        se_vega=out["se_vega"], se_rho=out["se_rho"], se_theta=out["se_theta"], se_epsilon=out["se_epsilon"],
        price_up=out["price_up"], price_down=out["price_down"], bump=out["bump"], n_paths=M,
        n_exercised=out["n_exercised"], n_exercised_up=out["n_exercised_up"], n_exercised_down=out["n_exercised_down"],
        sum_nitm=out["sum_nitm"], folded=bool(out["folded"]), dividend_steps=out["n_div_steps"],
        first_dividend_step=out["first_div_step"], dividend_yield=q, model=model_l, option_type=option_type,
        betas=out["betas"],
        timings_ms=dict(paths=out["ms_paths"], pass1=out["ms_pass1"], greeks=out["ms_greeks"], total=out["ms_total"]))


@dataclass
class JumpResult:
    """price_american_jumps: price / stderr (the convention of PriceResult), the exercise counts, the compensator
    kappa = E[e^J] - 1 and the drift rate (r - q) - lambda kappa the paths ran at."""
    price: float
    stderr: float
    std: float
    zero_prob: float
    n_paths: int
    n_exercised: int
    sum_nitm: int
    folded: bool
    kappa: float
    drift_rate: float
    jump_intensity: float
    jump_mean: float
    jump_vol: float
    dividend_yield: float
    model: str
    option_type: str
    timings_ms: dict = field(default_factory=dict)
    info: dict = field(default_factory=dict)  # max_jumps_per_step

    def __float__(self):
        return float(self.price)


def price_american_jumps(S0, K, r, sigma, T, n_paths, n_steps, jump_intensity, jump_mean=0.0, jump_vol=0.0,
                         dividend_yield=0.0, model="GBM", option_type="put", heston_params=None, seed=42,
                         device=None, heston_scheme="reference") -> JumpResult:
    """American option under jump-diffusion (omc_price_american_jump): the two-pass poly LSM of
    price_american_option on paths that carry compound-Poisson jumps -- jump_intensity jumps per year, each multiplying
    the spot by exp(J), J ~ N(jump_mean, jump_vol^2) -- and drift at r - dividend_yield - jump_intensity (E[e^J] - 1).
    model "GBM" is Merton's jump-diffusion, "Heston" is Bates's model.  jump_intensity * T / n_steps may not exceed 1.
    Antithetic paths, one GPU.
    heston_scheme (model="Heston"): "reference" (= "clamp"), "full_truncation", "calibrator", or "qe" -- Andersen's (2008)
    quadratic-exponential rule, which needs kappa > 0, theta > 0 and xi > 0 (ValueError otherwise).  With "qe" the jump multiplies the
    spot after the QE step (Bates on QE)."""
    model_l = str(model).lower()
    if model_l not in ("gbm", "heston"):
        raise ValueError("model must be 'GBM' or 'Heston'.")
    lam, mu, sj, q = _jump_args(jump_intensity, jump_mean, jump_vol, dividend_yield)
    _validate(S0, K, T, r, sigma, n_paths, n_steps, option_type, need_sigma=(model_l == "gbm"))
    _validate_scheme(model_l, heston_scheme, sigma, heston_params)
    if lam * float(T) / int(n_steps) > 1.0:
        raise ValueError("jump_intensity * T / n_steps must not exceed 1: use more time steps.")
    M = _even_paths(n_paths)
    c = _ffi.default_context(device)
    p = _ffi.make_params(model=model_l, is_put=(option_type == "put"), semantics="two_pass", antithetic=True,
                         n_paths=M, n_steps=int(n_steps), S0=S0, K=K, r=r, sigma=sigma or 0.0, T=T, seed=seed,
                         heston_scheme=heston_scheme, **heston_defaults(sigma, heston_params))
    out = c.price_american_jump(p, (lam, mu, sj), q)
    var = max(out["sumsq"] / M - out["price"] ** 2, 0.0)
    return JumpResult(price=out["price"], stderr=math.sqrt(var / M), std=out["std"], zero_prob=out["zero_prob"],
                      n_paths=M, n_exercised=out["n_exercised"], sum_nitm=out["sum_nitm"], folded=bool(out["folded"]),
                      kappa=out["kappa"], drift_rate=out["drift_rate"], jump_intensity=lam, jump_mean=mu, jump_vol=sj,
                      dividend_yield=q, model=model_l, option_type=option_type,
                      timings_ms=dict(paths=out["ms_jump_paths"], pass1=out["ms_pass1"], pass2=out["ms_pass2"],
                                      lsm=out["ms_lsm"], total=out["ms_total"]),
                      info=dict(max_jumps_per_step=out["n_thresholds"]))


@dataclass
class JumpGreeksResult:
    """price_american_jump_greeks: the frozen-policy price and its Greeks in raw units (per unit S0 / S0^2 / sigma / r / q /
    year / jump_intensity / jump_mean / jump_vol), their standard errors, the bumped scenarios and the policy used.
    theta_score is the score-function part of theta (already inside theta).  Heston (Bates): everything but delta and
    gamma is NaN; at jump_intensity = 0 dlambda is NaN."""
    price: float
    stderr: float
    delta: float
    gamma: float
    vega: float
    rho: float
    theta: float
    epsilon: float
    dlambda: float
    dmu_j: float
    dsigma_j: float
    theta_score: float
    se_delta: float
    se_gamma: float
    se_vega: float
    se_rho: float
    se_theta: float
    se_epsilon: float
    se_dlambda: float
    se_dmu_j: float
    se_dsigma_j: float
    se_theta_score: float
    price_up: float
    price_down: float
    bump: float
    n_paths: int
    n_exercised: int
    n_exercised_up: int
    n_exercised_down: int
    sum_nitm: int
    n_jumps: int
    kappa: float
    drift_rate: float
    jump_intensity: float
    jump_mean: float
    jump_vol: float
    dividend_yield: float
    model: str
    option_type: str
    betas: object = None  # numpy [n_steps+1][4]: b0, b1, b2, n
    timings_ms: dict = field(default_factory=dict)

    def __float__(self):
        return float(self.price)


def price_american_jump_greeks(S0, K, r, sigma, T, n_paths, n_steps, jump_intensity, jump_mean=0.0, jump_vol=0.0,
                               dividend_yield=0.0, model="GBM", option_type="put", heston_params=None,
                               heston_scheme="reference", seed=42, stream=0, bump=0.01, betas=None, device=None,
                               ctx=None) -> JumpGreeksResult:
    """Delta, gamma, vega, rho, theta, epsilon (dV/d dividend_yield) and the jump Greeks dlambda, dmu_j, dsigma_j
    (dV/d jump_intensity, jump_mean, jump_vol) of the American price price_american_jumps quotes, with the exercise policy
    pass 1 fits -- or `betas` [n_steps+1][4] -- held fixed (omc_price_american_jump_greeks).  One
    forward sweep regenerates the paths with their jump counts and sizes: with jumps the stored spot no longer gives the
    Brownian value price_american_greeks reads back from it.  A step's jump count is an integer, so dlambda and theta
    carry a score-function term next to their pathwise part; theta is -dV/dT at fixed n_steps.  Heston (Bates) gives
    delta and gamma; the others are NaN.  jump_intensity * T / n_steps may not exceed 1.  Antithetic paths, one GPU."""
    model_l = str(model).lower()
    if model_l not in ("gbm", "heston"):
        raise ValueError("model must be 'GBM' or 'Heston'.")
    lam, mu, sj, q = _jump_args(jump_intensity, jump_mean, jump_vol, dividend_yield)
    if not (0.0 < float(bump) <= 0.5):
        raise ValueError("bump must lie in (0, 0.5].")
    _validate(S0, K, T, r, sigma, n_paths, n_steps, option_type, need_sigma=(model_l == "gbm"))
    _validate_scheme(model_l, heston_scheme, sigma, heston_params)
    if lam * float(T) / int(n_steps) > 1.0:
        raise ValueError("jump_intensity * T / n_steps must not exceed 1: use more time steps.")
    M = _even_paths(n_paths)
    p = _ffi.make_params(model=model_l, is_put=(option_type == "put"), semantics="two_pass", antithetic=True,
                         n_paths=M, n_steps=int(n_steps), S0=S0, K=K, r=r, sigma=sigma or 0.0, T=T, seed=seed,
                         stream=stream, heston_scheme=heston_scheme, **heston_defaults(sigma, heston_params))
    c = ctx or _ffi.default_context(device)
    out = c.price_american_jump_greeks(p, (lam, mu, sj), q, bump=float(bump), betas=betas, want_betas=True)
    var = max(out["sumsq"] / M - out["price"] ** 2, 0.0)
    names = ("delta", "gamma", "vega", "rho", "theta", "epsilon", "dlambda", "dmu_j", "dsigma_j", "theta_score")
    return JumpGreeksResult(
        price=out["price"], stderr=math.sqrt(var / M), **{k: out[k] for k in names},
        **{"se_" + k: out["se_" + k] for k in names},
        price_up=out["price_up"], price_down=out["price_down"], bump=out["bump"], n_paths=M,
        n_exercised=out["n_exercised"], n_exercised_up=out["n_exercised_up"], n_exercised_down=out["n_exercised_down"],
        sum_nitm=out["sum_nitm"], n_jumps=out["n_jumps"], kappa=out["kappa"], drift_rate=out["drift_rate"],
        jump_intensity=lam, jump_mean=mu, jump_vol=sj, dividend_yield=q, model=model_l, option_type=option_type,
        betas=out["betas"],
        timings_ms=dict(paths=out["ms_paths"], pass1=out["ms_pass1"], greeks=out["ms_greeks"], total=out["ms_total"]))


@dataclass
class BasketResult:
    """price_american_basket: price / stderr (the convention of PriceResult), the exercise counts and the index of the
    initial spots.  The exercise policy behind the price is a function of the INDEX alone."""
    price: float
    stderr: float
    std: float
    zero_prob: float
    n_paths: int
    n_exercised: int
    sum_nitm: int
    index0: float
    n_assets: int
    kind: str
    option_type: str
    timings_ms: dict = field(default_factory=dict)
    info: dict = field(default_factory=dict)  # weights, geometric (G0, sigma_G, q_G)

    def __float__(self):
        return float(self.price)


_BASKET_KINDS = ("basket", "geometric", "best-of", "worst-of", "asian", "asian-geometric")


def _basket_args(spots, sigmas, weights, dividend_yields, correlation, kind):
    """The per-asset arguments of the multi-asset entry points, checked and with their defaults -> (S0, sigma, q, w, rho)."""
    if kind not in _BASKET_KINDS:
        raise ValueError(f"kind must be one of {list(_BASKET_KINDS)}.")
    try:
        S0 = [float(x) for x in spots]
        sig = [float(x) for x in sigmas]
    except TypeError:
        raise ValueError("spots and sigmas must be sequences with one entry per asset.") from None
    d = len(S0)
    if not 1 <= d <= _ffi.BASKET_MAX_ASSETS:
        raise ValueError(f"a basket has 1 .. {_ffi.BASKET_MAX_ASSETS} assets.")
    if len(sig) != d:
        raise ValueError("sigmas must have one entry per asset.")
    w = [1.0 / d if kind in ("basket", "geometric", "asian", "asian-geometric") else 1.0] * d if weights is None else [float(x) for x in weights]
    q = [0.0] * d if dividend_yields is None else [float(x) for x in dividend_yields]
    if len(w) != d or len(q) != d:
        raise ValueError("weights and dividend_yields must have one entry per asset.")
    if not all(math.isfinite(x) and x > 0.0 for x in S0):
        raise ValueError("every spot must be finite and positive.")
    if not all(math.isfinite(x) and x > 0.0 for x in sig):
        raise ValueError("every sigma must be finite and positive.")
    if not all(math.isfinite(x) and x > 0.0 for x in w):
        raise ValueError("every weight must be finite and positive.")
    if not all(math.isfinite(x) for x in q):
        raise ValueError("every dividend yield must be finite.")
    rho = [[1.0 if i == j else 0.0 for j in range(d)] for i in range(d)] if correlation is None else \
        [[float(x) for x in row] for row in correlation]
    if len(rho) != d or any(len(row) != d for row in rho):
        raise ValueError(f"correlation must be a {d} x {d} matrix.")
    return S0, sig, q, w, rho


def price_american_basket(spots, K, r, sigmas, T, n_paths, n_steps, correlation=None, weights=None, dividend_yields=None,
                          kind="basket", option_type="put", seed=None, device=None) -> BasketResult:
    """American option on an index of 1 .. 8 correlated GBM assets (omc_price_american_basket): the
    two-pass poly LSM of price_american_option on the matrix of the index X_t -- kind "basket" sum w_i S_i, "geometric"
    prod S_i^w_i, "best-of" max w_i S_i, "worst-of" min w_i S_i -- with the payoff max(K - X, 0) or max(X - K, 0).  The
    regression is on the index, so the exercise policy is a function of the index alone: the usual dominant regressor for
    baskets, a deliberately simple policy for best-of / worst-of.  correlation: [d][d], default identity; weights: default
    1 / d for "basket" and "geometric", 1 for "best-of" and "worst-of"; dividend_yields: default 0; seed: default 42.
    kind "asian" / "asian-geometric" (DESIGN.md section 23): the index is the running arithmetic / geometric average over
    the grid dates 1 .. t of the basket value sum w_i S_i -- a fixed-strike average-price option with early exercise; with
    one asset of weight 1 the plain Asian option (price_asian_option).
    The flow is the reference's two-pass rule: not comparable with tables of textbook LSM.
    Antithetic paths, one GPU."""
    S0, sig, q, w, rho = _basket_args(spots, sigmas, weights, dividend_yields, correlation, kind)
    d = len(S0)
    _validate(S0[0], K, T, r, sig[0], n_paths, n_steps, option_type)
    M = _even_paths(n_paths)
    p = _ffi.make_params(model="gbm", is_put=(option_type == "put"), semantics="two_pass", antithetic=True, n_paths=M,
                         n_steps=int(n_steps), S0=S0[0], K=K, r=r, sigma=sig[0], T=T, seed=42 if seed is None else int(seed))
    b = _ffi.make_basket(S0, sig, q, w, rho, kind)
    _, _, _, _, geo = _ffi.basket_table(p, b)  # host only: the library's own checks (the correlation matrix among them)
    c = _ffi.default_context(device)
    out = c.price_american_basket(p, b)
    var = max(out["sumsq"] / M - out["price"] ** 2, 0.0)
    return BasketResult(price=out["price"], stderr=math.sqrt(var / M), std=out["std"], zero_prob=out["zero_prob"],
                        n_paths=M, n_exercised=out["n_exercised"], sum_nitm=out["sum_nitm"], index0=out["index0"],
                        n_assets=d, kind=kind, option_type=option_type,
                        timings_ms=dict(paths=out["ms_basket_paths"], pass1=out["ms_pass1"], pass2=out["ms_pass2"],
                                        lsm=out["ms_lsm"], total=out["ms_total"]),
                        info=dict(weights=w, geometric=dict(G0=geo[0], sigma_G=geo[1], q_G=geo[2])))


@dataclass
class BasketGreeksResult:
    """price_american_basket_greeks: the price of price_american_basket and its frozen-policy pathwise Greeks -- delta,
    gamma (diagonal) and vega per asset, rho and theta of the option -- in raw units (per unit S0_i / S0_i^2 / sigma_i /
    r / year), with their standard errors.  price_up[i] / price_down[i]: the frozen-policy prices at S0_i (1 +- bump)."""
    price: float
    stderr: float
    delta: list
    gamma: list
    vega: list
    rho: float
    theta: float
    se_delta: list
    se_gamma: list
    se_vega: list
    se_rho: float
    se_theta: float
    price_up: list
    price_down: list
    bump: float
    n_paths: int
    n_exercised: int
    index0: float
    n_assets: int
    kind: str
    option_type: str
    betas: object = None
    timings_ms: dict = field(default_factory=dict)
    info: dict = field(default_factory=dict)  # weights

    def __float__(self):
        return float(self.price)


def price_american_basket_greeks(spots, K, r, sigmas, T, n_paths, n_steps, correlation=None, weights=None,
                                 dividend_yields=None, kind="basket", option_type="put", bump=0.01, gamma=True, betas=None,
                                 seed=None, device=None, ctx=None, n_gpus=1) -> BasketGreeksResult:
    """Per-asset delta, diagonal gamma and vega, and rho and theta, of the price of price_american_basket with the
    exercise policy pass 1 fits held fixed (omc_price_american_basket_greeks): the assets, kinds and
    defaults of price_american_basket.  They are exact derivatives of that frozen-policy estimator.  gamma[i] is a central
    difference of pathwise deltas with asset i alone at S0_i (1 +- bump) on the same normals; gamma=False skips it.
    betas ([n_steps+1][4] = b0, b1, b2, n): a given policy instead of the fitted one; an all-zero table gives the Greeks
    of the European option.  Antithetic paths, one GPU."""
    if int(n_gpus) != 1:
        raise ValueError("price_american_basket_greeks runs on one GPU (n_gpus=1).")
    if not (0.0 < float(bump) <= 0.5):
        raise ValueError("bump must lie in (0, 0.5].")
    S0, sig, q, w, rho = _basket_args(spots, sigmas, weights, dividend_yields, correlation, kind)
    d = len(S0)
    _validate(S0[0], K, T, r, sig[0], n_paths, n_steps, option_type)
    M = _even_paths(n_paths)
    if betas is not None and np.asarray(betas).shape != (int(n_steps) + 1, 4):
        raise ValueError(f"betas must have shape ({int(n_steps) + 1}, 4).")
    p = _ffi.make_params(model="gbm", is_put=(option_type == "put"), semantics="two_pass", antithetic=True, n_paths=M,
                         n_steps=int(n_steps), S0=S0[0], K=K, r=r, sigma=sig[0], T=T, seed=42 if seed is None else int(seed))
    b = _ffi.make_basket(S0, sig, q, w, rho, kind)
    _ffi.basket_table(p, b)  # host only: the library's own checks (the correlation matrix among them)
    c = ctx or _ffi.default_context(device)
    out = c.price_american_basket_greeks(p, b, bump=float(bump), gamma=bool(gamma), betas=betas, want_betas=True)
    var = max(out["sumsq"] / M - out["price"] ** 2, 0.0)
    return BasketGreeksResult(price=out["price"], stderr=math.sqrt(var / M), delta=out["delta"], gamma=out["gamma"],
                              vega=out["vega"], rho=out["rho"], theta=out["theta"], se_delta=out["se_delta"],
                              se_gamma=out["se_gamma"], se_vega=out["se_vega"], se_rho=out["se_rho"],
                              se_theta=out["se_theta"], price_up=out["price_up"], price_down=out["price_down"],
                              bump=out["bump"], n_paths=M, n_exercised=out["n_exercised"], index0=out["index0"],
                              n_assets=d, kind=kind, option_type=option_type, betas=out["betas"],
                              timings_ms=dict(paths=out["ms_basket_paths"], pass1=out["ms_pass1"], greeks=out["ms_greeks"],
                                              total=out["ms_total"]),
                              info=dict(weights=w))


@dataclass
class BoundsResult:
    """price_american_bounds: Andersen-Broadie bounds on the value of the BERMUDAN option with exercise dates t = 1..n_steps
    of the grid dt = T / n_steps, all values discounted to t = 0 (Z_t = exp(-r t dt) max(phi(S_t), 0)) -- the textbook
    convention, not the t = dt valuation of the library's reference and two_pass flows -- from one frozen exercise policy
    `betas` ([n_steps+1][4] = b0, b1, b2, n).  `lower` applies the policy as a stopping rule on fresh paths; `upper` is the
    dual estimator with nested inner simulations (biased upward only).  [ci_lo, ci_hi] = [lower - 1.96 se_lower,
    upper + 1.96 se_upper].  They bound the game on the grid, not the continuously exercisable American option."""
    lower: float
    se_lower: float
    upper: float
    se_upper: float
    ci_lo: float
    ci_hi: float
    n_lower: int
    n_outer: int
    n_inner: int
    n_exercised_lower: int
    inner_path_steps: int
    policy: str
    betas: object
    option_type: str
    timings_ms: dict = field(default_factory=dict)
    exercise_every: int = 0  # 0 = every date of the grid; k >= 2: every k-th date counted back from expiry (section 25)
    n_exercise_dates: int = 0  # the dates of the game, the expiry included (0: not recorded)
    control_variate: bool = False  # the Black-Scholes control variate of the GBM bounds (section 26)
    suboptimality_check: str = "off"  # "payoff" / "european": inner simulations at the kept items only (section 27)


# The argument checks that the bounds facades share, as stages: each facade calls them where its own order of refusals has
# them, between its own law's checks.

def _model_name(model):
    model_l = str(model).lower()
    if model_l not in ("gbm", "heston"):
        raise ValueError("model must be 'GBM' or 'Heston'.")
    return model_l


def _true_or_false(control_variate):
    if not isinstance(control_variate, (bool, int)) or control_variate not in (0, 1):
        raise ValueError("control_variate must be True or False.")


def _bounds_sizes(policy, betas, n_lower, n_outer, n_inner):
    """the policy's name, `betas` exactly with policy "given", and the three sizes in whole antithetic pairs"""
    if policy not in _ffi.BOUND_POLICIES:
        raise ValueError(f"policy must be one of {sorted(_ffi.BOUND_POLICIES)}.")
    if (policy == "given") != (betas is not None):
        raise ValueError("betas must be given exactly when policy='given'.")
    for name, v in (("n_lower", n_lower), ("n_outer", n_outer), ("n_inner", n_inner)):
        if int(v) < 2 or int(v) % 2:
            raise ValueError(f"{name} must be an even integer >= 2 (antithetic pairs).")


# law -> whose bounds have no control variate, who takes 'payoff' or 'off', and whose price bounds take two schemes
_LAW_WORDS = {"heston": (None, None, "under Heston"),
              "jump": ("jump-diffusion", "jump-diffusion takes", "under Bates"),
              "dividend": ("dividend", "dividends take", "with dividends"),
              "barrier": ("barrier", "barrier options take", "of barrier options")}


def _bounds_switches(law, control_variate, suboptimality_check, exercise_every):
    """What the jump, dividend and barrier laws refuse of the switches of price_american_bounds -- the control variate and
    the "european" check -- then the check's name and the schedule -> exercise_every as an int."""
    no_cv, payoff_or_off, _ = _LAW_WORDS[law]
    if control_variate:
        raise ValueError(f"control_variate: the {no_cv} bounds have no control variate.")
    if suboptimality_check == "european":
        raise ValueError(f"suboptimality_check='european' is for price_american_bounds only ({payoff_or_off} 'payoff' or "
                         "'off').")
    if suboptimality_check is not None and suboptimality_check not in _ffi.BOUND_CHECKS:
        raise ValueError(f"suboptimality_check must be one of {list(_ffi.BOUND_CHECKS)} or None.")
    every = _one_schedule(exercise_every)
    if every >= 2 and suboptimality_check == "payoff":
        raise ValueError("sub-optimality checking is for the game on every date (exercise_every must be 0 or 1).")
    return every


def _bounds_scheme(law, model_l, heston_scheme):
    """The bounds run on Heston scheme "reference" (= "clamp") or "full_truncation"; price_american_bounds_heston also says
    which scheme it was given."""
    if model_l != "heston":
        return
    if heston_scheme not in _ffi.HESTON_SCHEMES:
        raise ValueError(f"heston_scheme must be one of {sorted(_ffi.HESTON_SCHEMES)}.")
    if _ffi.HESTON_SCHEMES[heston_scheme] not in (_ffi.HESTON_SCHEMES["reference"], _ffi.HESTON_SCHEMES["full_truncation"]):
        raise ValueError(f"price bounds {_LAW_WORDS[law][2]} take heston_scheme 'reference' or 'full_truncation'"
                         + (f", not '{heston_scheme}'." if law == "heston" else "."))


def _betas_shape(betas, n_steps, cols):
    if betas is not None and np.shape(betas) != (int(n_steps) + 1, cols):
        raise ValueError(f"betas must have shape ({int(n_steps) + 1}, {cols}), got {np.shape(betas)}.")


def _law_params(model_l, option_type, heston_scheme, heston_params, M, n_steps, S0, K, r, sigma, T, seed, stream):
    """omc_params of a one-asset bounds call: two-pass flow, M antithetic paths, GBM or Heston"""
    if model_l == "heston":
        return _ffi.make_params(model="heston", is_put=(option_type == "put"), semantics="two_pass", antithetic=True,
                                heston_scheme=heston_scheme, n_paths=M, n_steps=int(n_steps), S0=S0, K=K, r=r,
                                sigma=sigma or 0.0, T=T, seed=seed, stream=stream, **heston_defaults(sigma, heston_params))
    return _ffi.make_params(is_put=(option_type == "put"), semantics="two_pass", antithetic=True, n_paths=M,
                            n_steps=int(n_steps), S0=S0, K=K, r=r, sigma=sigma, T=T, seed=seed, stream=stream)


def _game(n_steps, every):
    """the schedule's two fields of a BoundsResult"""
    return dict(exercise_every=every, n_exercise_dates=len(bounds_exercise_dates(n_steps, every)))


def _bounds_result(cls, out, *, policy, option_type, **law_fields):
    """The dict of a Context.price_*bounds* call as `cls`: the fields every law has, then the facade's own."""
    return cls(lower=out["lower"], se_lower=out["se_lower"], upper=out["upper"], se_upper=out["se_upper"],
               ci_lo=out["ci_lo"], ci_hi=out["ci_hi"], n_lower=out["n_lower"], n_outer=out["n_outer"], n_inner=out["n_inner"],
               n_exercised_lower=out["n_exercised_lower"], inner_path_steps=out["inner_path_steps"], policy=policy,
               betas=out["betas"], option_type=option_type,
               timings_ms=dict(fit=out["ms_fit"], lower=out["ms_lower"], upper=out["ms_upper"], total=out["ms_total"]),
               **law_fields)


def price_american_bounds(S0, K, r, sigma, T, n_paths, n_steps, option_type="put", policy="textbook", n_lower=1_000_000,
                          n_outer=8192, n_inner=1024, seed=42, stream=0, betas=None, device=None,
                          ctx=None, control_variate=False, exercise_every=0) -> BoundsResult:
    """Lower and upper bounds on the Bermudan value of a GBM put / call (omc_price_american_bounds).
    policy: "textbook" (classic Longstaff-Schwartz fits, the best of the library's policies), "two_pass" or "reference"
    (the fits of the headline flows), each fitted on n_paths paths at (seed, stream); or "given" with `betas`
    [n_steps+1][4].  The lower-bound, outer and inner paths use Philox streams stream + 1, + 2, + 3.  One GPU.
    exercise_every = k >= 2: the bounds of the game with exercise at every k-th date counted back
    from expiry, and at expiry, on paths of the whole grid; `betas` then has zero rows off the schedule.
    control_variate=True: the same paths and stops with the discounted Black-Scholes value of the
    European option as a control variate in the lower bound and in every inner mean -- far smaller standard errors, and an
    upper bound whose bias a small n_inner no longer inflates."""
    every = _one_schedule(exercise_every)
    _true_or_false(control_variate)
    _bounds_sizes(policy, betas, n_lower, n_outer, n_inner)
    _validate(S0, K, T, r, sigma, n_paths, n_steps, option_type)
    M = _even_paths(n_paths)
    c = ctx or _ffi.default_context(device)
    p = _law_params("gbm", option_type, None, None, M, n_steps, S0, K, r, sigma, T, seed, stream)
    out = c.price_american_bounds(p, policy=policy, n_lower=int(n_lower), n_outer=int(n_outer), n_inner=int(n_inner),
                                  betas=betas, exercise_every=every, control_variate=bool(control_variate))
    return _bounds_result(BoundsResult, out, policy=policy, option_type=option_type, **_game(n_steps, every),
                          control_variate=bool(control_variate))


@dataclass
class HestonBoundsResult(BoundsResult):
    """price_american_bounds_heston: BoundsResult with what the policy saw.  With regressors "spot" the policy is a function
    of the spot alone; with "spot+variance" of the spot and the variance state (`betas` is then [n_steps+1][8] = c0 .. c5,
    n, 0, and its w is V / variance_scale - 1 with variance_scale = max(v0, theta)).  `lower` is what that policy earns,
    `upper` bounds the value of the discretised scheme's game under ANY policy."""
    regressors: str = "spot"
    variance_scale: float = 0.0


def price_american_bounds_heston(S0, K, r, T, n_paths, n_steps, heston_params=None, heston_scheme="reference",
                                 option_type="put", policy="textbook", n_lower=1_000_000, n_outer=8192, n_inner=1024,
                                 seed=42, stream=0, betas=None, device=None, ctx=None,
                                 regressors="spot", exercise_every=0) -> HestonBoundsResult:
    """Lower and upper bounds on the Bermudan value of a put / call under the Heston model
    (omc_price_american_bounds_heston): price_american_bounds with Heston paths.  heston_params as
    price_american_option takes them (v0, kappa, theta, xi, rho; the defaults of heston_defaults at sigma = 0.2);
    heston_scheme "reference" (= "clamp") or "full_truncation" -- the calibrator's scheme and "qe" have no bounds.  The policy
    (`policy` / `betas` as price_american_bounds takes them) regresses on the spot alone; the inner simulations start at the
    outer paths' (spot, variance) state, so `upper` bounds the value under any policy of the DISCRETISED scheme's game on
    the grid, one that sees the variance included.  The lower-bound, outer and inner paths use Philox streams stream + 1,
    + 2, + 3.  One GPU.
    regressors="spot+variance" (DESIGN.md section 21): the policy also sees the variance state, the other half of the Markov
    state, as w = V / max(v0, theta) - 1 (`variance_scale` of the result: a scale for conditioning only, which a `given`
    table must share).  policy is then "textbook" or "given", n_steps at most 512, and `betas` is [n_steps+1][8] = c0, c1,
    c2 (1, u, u^2 of the spot), c3, c4 (w, w^2 of the variance), c5 (u w), n, 0.
    exercise_every = k >= 2: as price_american_bounds takes it, with regressors "spot" only."""
    every = _one_schedule(exercise_every)
    if every >= 2 and regressors == "spot+variance":
        raise ValueError("the spot + variance policy takes no exercise schedule (exercise_every must be 0 or 1).")
    _bounds_sizes(policy, betas, n_lower, n_outer, n_inner)
    _bounds_scheme("heston", "heston", heston_scheme)
    _validate(S0, K, T, r, None, n_paths, n_steps, option_type, need_sigma=False)
    M = _even_paths(n_paths)
    hp = heston_defaults(None, heston_params)
    _ffi.check_heston_regressors(regressors, policy, n_steps, hp["v0"], hp["theta"])
    _betas_shape(betas, n_steps, 8 if regressors == "spot+variance" else 4)
    p = _law_params("heston", option_type, heston_scheme, hp, M, n_steps, S0, K, r, None, T, seed, stream)
    c = ctx or _ffi.default_context(device)
    out = c.price_american_bounds_heston(p, policy=policy, n_lower=int(n_lower), n_outer=int(n_outer),
                                         n_inner=int(n_inner), betas=betas, regressors=regressors, exercise_every=every)
    return _bounds_result(HestonBoundsResult, out, policy=policy, option_type=option_type, regressors=regressors,
                          variance_scale=max(float(hp["v0"]), float(hp["theta"])), **_game(n_steps, every))


class ChainBoundsResult(list):
    """price_american_chain_bounds: one BoundsResult (HestonBoundsResult under Heston) per quote, in the caller's order,
    and what the chain as a whole did: `inner_path_steps_simulated` (the steps its inner pairs were simulated for -- at least
    the largest and at most the sum of the entries' inner_path_steps), `n_groups` (the entries ride on one simulation in
    groups of at most `entries_per_group`) and `timings_ms` (fit, lower, upper, total of the whole call)."""

    def __init__(self, entries, strikes, option_types, inner_path_steps_simulated, n_groups, entries_per_group, timings_ms):
        super().__init__(entries)
        self.strikes = strikes
        self.option_types = option_types
        self.inner_path_steps_simulated = inner_path_steps_simulated
        self.n_groups = n_groups
        self.entries_per_group = entries_per_group
        self.timings_ms = timings_ms


def _chain_quotes(strikes, option_types):
    """strikes / option_types of a chain -> the strikes as floats and one side per strike (ValueError otherwise)"""
    try:
        ks = [float(k) for k in strikes]
    except TypeError:
        raise ValueError("strikes must be a sequence of numbers.") from None
    if not ks:
        raise ValueError("strikes must not be empty.")
    if len(ks) > _ffi.CHAIN_MAX:
        raise ValueError(f"a chain has at most {_ffi.CHAIN_MAX} entries.")
    types = [option_types] * len(ks) if isinstance(option_types, str) else list(option_types)
    if len(types) != len(ks):
        raise ValueError("option_types must be one string or one per strike.")
    return ks, types


def price_american_chain_bounds(S0, strikes, r, sigma, T, n_paths, n_steps, option_types="put", model="GBM",
                                heston_params=None, heston_scheme="reference", policy="textbook", n_lower=1_000_000,
                                n_outer=8192, n_inner=1024, seed=42, stream=0, betas=None, device=None,
                                ctx=None) -> ChainBoundsResult:
    """Lower and upper bounds for every quote of one expiry -- `strikes`, each a put or a call (`option_types`: one string
    for all, or one per strike) -- from ONE set of fitting, lower-bound, outer and inner paths
    (omc_price_american_chain_bounds).  Entry i equals price_american_bounds(S0, strikes[i], ...,
    option_type=option_types[i]) -- under model="Heston" price_american_bounds_heston with regressors "spot" -- at the same
    sizes, seed and stream: bit for bit in betas, lower, se_lower, n_exercised_lower and inner_path_steps, and in upper and
    se_upper while n_inner <= 128; beyond, upper differs by the order of float64 sums.  policy as
    price_american_bounds takes it; with "given", `betas` is [len(strikes)][n_steps+1][4].  heston_scheme "reference"
    (= "clamp") or "full_truncation".  No exercise schedule, control variate or sub-optimality check.  One GPU."""
    model_l = _model_name(model)
    ks, types = _chain_quotes(strikes, option_types)
    _bounds_sizes(policy, betas, n_lower, n_outer, n_inner)
    _bounds_scheme("heston", model_l, heston_scheme)
    heston = model_l == "heston"
    for k, ot in zip(ks, types):
        if not (math.isfinite(k) and k > 0):
            raise ValueError("S0, K, T must be positive.")
        _validate(S0, k, T, r, None if heston else sigma, n_paths, n_steps, ot, need_sigma=not heston)
    if betas is not None and np.shape(betas) != (len(ks), int(n_steps) + 1, 4):
        raise ValueError(f"betas must have shape ({len(ks)}, {int(n_steps) + 1}, 4), got {np.shape(betas)}.")
    M = _even_paths(n_paths)
    hp = heston_defaults(None, heston_params) if heston else None
    p = _law_params(model_l, types[0], heston_scheme, hp, M, n_steps, S0, ks[0], r, None if heston else sigma, T, seed, stream)
    c = ctx or _ffi.default_context(device)
    outs, info = c.price_american_chain_bounds(p, ks, [ot == "put" for ot in types], policy=policy, n_lower=int(n_lower),
                                               n_outer=int(n_outer), n_inner=int(n_inner), betas=betas)
    if heston:
        law = dict(regressors="spot", variance_scale=max(float(hp["v0"]), float(hp["theta"])))
        entries = [_bounds_result(HestonBoundsResult, out, policy=policy, option_type=ot, **law, **_game(n_steps, 0))
                   for out, ot in zip(outs, types)]
    else:
        entries = [_bounds_result(BoundsResult, out, policy=policy, option_type=ot, **_game(n_steps, 0))
                   for out, ot in zip(outs, types)]
    return ChainBoundsResult(entries, ks, types, info["inner_path_steps_simulated"], info["n_groups"],
                             info["entries_per_group"],
                             dict(fit=info["ms_fit"], lower=info["ms_lower"], upper=info["ms_upper"], total=info["ms_total"]))


@dataclass
class JumpBoundsResult(BoundsResult):
    """price_american_bounds_jumps: BoundsResult with the jump law.  The policy is a function of the spot alone; `lower` is
    what it earns, `upper` bounds the value of the discretised jump-diffusion's game on the grid under ANY policy."""
    jump_intensity: float = 0.0
    jump_mean: float = 0.0
    jump_vol: float = 0.0
    dividend_yield: float = 0.0
    model: str = "gbm"


def price_american_bounds_jumps(S0, K, r, sigma, T, n_paths, n_steps, jump_intensity, jump_mean=0.0, jump_vol=0.0,
                                dividend_yield=0.0, model="GBM", option_type="put", policy="textbook", n_lower=1_000_000,
                                n_outer=8192, n_inner=1024, heston_params=None, heston_scheme="reference", seed=42, stream=0,
                                betas=None, exercise_every=0, suboptimality_check=None, device=None, ctx=None,
                                control_variate=False) -> JumpBoundsResult:
    """Lower and upper bounds on the Bermudan value of a put / call under jump-diffusion (omc_price_american_bounds_jump,
    DESIGN.md section 28): price_american_bounds on the paths of price_american_jumps -- jump_intensity jumps per year, each
    multiplying the spot by exp(J), J ~ N(jump_mean, jump_vol^2), drift at r - dividend_yield - jump_intensity (E[e^J] - 1),
    discounting at r.  model "GBM" is Merton's jump-diffusion, "Heston" is Bates's model (heston_params as
    price_american_option takes them; heston_scheme "reference" (= "clamp") or "full_truncation").  jump_intensity * T /
    n_steps may not exceed 1.  The policy (`policy` / `betas` as price_american_bounds takes them) regresses on the spot alone;
    the inner simulations start at the outer paths' spot (Merton) or (spot, variance) state (Bates) -- the jumps are
    independent of the past, so that is the whole Markov state and `upper` bounds the value of the discretised game on the
    grid under any policy.  The bracket for the quote of price_american_jumps, which is a two-pass-flow value and lies above
    `upper`.  The lower-bound, outer and inner paths use Philox streams stream + 1, + 2, + 3.  One GPU.
    exercise_every = k >= 2: as price_american_bounds takes it.
    suboptimality_check: None / "off", or "payoff" (DESIGN.md section 27); "european" and control_variate=True need the
    European value under jumps per item and are refused."""
    model_l = _model_name(model)
    every = _bounds_switches("jump", control_variate, suboptimality_check, exercise_every)
    lam, mu, sj, q = _jump_args(jump_intensity, jump_mean, jump_vol, dividend_yield)
    _bounds_sizes(policy, betas, n_lower, n_outer, n_inner)
    _validate(S0, K, T, r, sigma, n_paths, n_steps, option_type, need_sigma=(model_l == "gbm"))
    _bounds_scheme("jump", model_l, heston_scheme)
    if lam * float(T) / int(n_steps) > 1.0:
        raise ValueError("jump_intensity * T / n_steps must not exceed 1: use more time steps.")
    M = _even_paths(n_paths)
    p = _law_params(model_l, option_type, heston_scheme, heston_params, M, n_steps, S0, K, r, sigma, T, seed, stream)
    c = ctx or _ffi.default_context(device)
    out = c.price_american_bounds_jump(p, (lam, mu, sj), q, policy=policy, n_lower=int(n_lower), n_outer=int(n_outer),
                                       n_inner=int(n_inner), betas=betas, exercise_every=every,
                                       suboptimality_check=suboptimality_check)
    return _bounds_result(JumpBoundsResult, out, policy=policy, option_type=option_type, **_game(n_steps, every),
                          suboptimality_check=suboptimality_check or "off", jump_intensity=lam, jump_mean=mu, jump_vol=sj,
                          dividend_yield=q, model=model_l)


@dataclass
class DividendBoundsResult(BoundsResult):
    """price_american_bounds_dividends: BoundsResult with the dividend law.  The policy is a function of the spot alone;
    `lower` is what it earns, `upper` bounds the value of the discretised game on the grid -- exercise at a dividend step
    earns the ex-dividend payoff -- under ANY policy."""
    dividend_yield: float = 0.0
    n_div_steps: int = 0     # time steps on which at least one dividend goes ex
    first_div_step: int = 0  # the first of them (0: none)
    model: str = "gbm"


def price_american_bounds_dividends(S0, K, r, sigma, T, n_paths, n_steps, dividend_yield=0.0, dividends=(), model="GBM",
                                    option_type="put", policy="textbook", n_lower=1_000_000, n_outer=8192, n_inner=1024,
                                    heston_params=None, heston_scheme="reference", seed=42, stream=0, betas=None,
                                    exercise_every=0, suboptimality_check=None, device=None, ctx=None,
                                    control_variate=False) -> DividendBoundsResult:
    """Lower and upper bounds on the Bermudan value of a put / call on a stock that pays dividends
    (omc_price_american_bounds_div): price_american_bounds on the paths of price_american_dividends --
    drift at r - dividend_yield, discounting at r, and on every ex-dividend step the spot drops by the dividend; exercise at
    that step earns the ex-dividend payoff.  dividends: the items price_american_dividends takes.  model "GBM" or "Heston"
    (heston_params as price_american_option takes them; heston_scheme "reference" (= "clamp") or "full_truncation").  The
    policy (`policy` / `betas` as price_american_bounds takes them) regresses on the spot alone; the inner simulations start
    at the outer paths' spot (GBM) or (spot, variance) state (Heston) and at their date -- with a deterministic schedule that
    is the whole Markov state, so `upper` bounds the value of the discretised game on the grid under any policy.  The
    bracket for the quote of price_american_dividends, which is a two-pass-flow value.  The lower-bound, outer and inner
    paths use Philox streams stream + 1, + 2, + 3.  One GPU.
    exercise_every = k >= 2: as price_american_bounds takes it.
    suboptimality_check: None / "off", or "payoff" (DESIGN.md section 27); "european" and control_variate=True are refused:
    the Black-Scholes value is not the European value after a cash dividend."""
    model_l = _model_name(model)
    every = _bounds_switches("dividend", control_variate, suboptimality_check, exercise_every)
    q = float(dividend_yield)
    if not math.isfinite(q):
        raise ValueError("dividend_yield must be finite.")
    divs = _dividend_items(dividends)
    _bounds_sizes(policy, betas, n_lower, n_outer, n_inner)
    _validate(S0, K, T, r, sigma, n_paths, n_steps, option_type, need_sigma=(model_l == "gbm"))
    _bounds_scheme("dividend", model_l, heston_scheme)
    M = _even_paths(n_paths)
    p = _law_params(model_l, option_type, heston_scheme, heston_params, M, n_steps, S0, K, r, sigma, T, seed, stream)
    has = _ffi.dividend_schedule(p, q, divs)[2]  # (host only: the library's own checks of the schedule, before a context)
    c = ctx or _ffi.default_context(device)
    out = c.price_american_bounds_div(p, q, divs, policy=policy, n_lower=int(n_lower), n_outer=int(n_outer),
                                      n_inner=int(n_inner), betas=betas, exercise_every=every,
                                      suboptimality_check=suboptimality_check)
    return _bounds_result(DividendBoundsResult, out, policy=policy, option_type=option_type, **_game(n_steps, every),
                          suboptimality_check=suboptimality_check or "off", dividend_yield=q, n_div_steps=int(has.sum()),
                          first_div_step=int(has.argmax()) if has.any() else 0, model=model_l)


@dataclass
class BarrierBoundsResult(BoundsResult):
    """price_barrier_bounds: BoundsResult for an American barrier option.  The policy is a function of the ENCODED index --
    the spot where the option is live, a dead spot elsewhere, so it never exercises a dead option; `lower` is what it
    earns, `upper` bounds the value of the discretised game on the grid under ANY policy that sees the path's state (spot,
    knocked yes / no, and under Heston the variance)."""
    barrier: float = 0.0
    barrier_type: str = "down-and-out"
    monitoring: str = "discrete"
    model: str = "gbm"


def price_barrier_bounds(S0, K, r, sigma, T, n_paths, n_steps, barrier, barrier_type="down-and-out", option_type="put",
                         model="GBM", heston_params=None, heston_scheme="reference", policy="textbook", exercise_every=0,
                         suboptimality_check=None, n_lower=1_000_000, n_outer=8192, n_inner=1024, seed=42, stream=0,
                         betas=None, device=None, ctx=None, monitoring="discrete",
                         control_variate=False) -> BarrierBoundsResult:
    """Lower and upper bounds on the value of the American knock-in / knock-out option that price_barrier_option quotes
    (omc_price_american_bounds_barrier): price_american_bounds on the barrier generator's paths.
    The barrier is monitored on every step of the grid (discrete monitoring); a knock-out is dead at its hit step and
    after it, a knock-in is live from its hit step on; no rebate.  model "GBM" or "Heston" (heston_params as
    price_american_option takes them; heston_scheme "reference" (= "clamp") or "full_truncation").  The policy (`policy` /
    `betas` as price_american_bounds takes them) is fitted on the encoded matrix price_barrier_option prices; the inner
    simulations start at the outer paths' (spot, knocked yes / no[, variance]) state.  The bracket for the quote of
    price_barrier_option, which is a two-pass-flow value.  The lower-bound, outer and inner paths use Philox streams
    stream + 1, + 2, + 3.  One GPU.
    exercise_every = k >= 2: as price_american_bounds takes it; the barrier stays monitored on every
    step, so daily monitoring with monthly exercise is exercise_every = 21 on a daily grid.
    suboptimality_check: None / "off", or "payoff" (DESIGN.md section 27); "european" and control_variate=True are refused:
    a vanilla European value is no bound on a barrier continuation value."""
    model_l = _model_name(model)
    if barrier_type not in _ffi.BARRIER_KINDS:
        raise ValueError(f"barrier_type must be one of {sorted(_ffi.BARRIER_KINDS)}.")
    if monitoring != "discrete":
        raise ValueError("monitoring: the barrier bounds take 'discrete' monitoring only.")
    every = _bounds_switches("barrier", control_variate, suboptimality_check, exercise_every)
    H = float(barrier)
    if not (math.isfinite(H) and H > 0):
        raise ValueError("barrier H must be finite and positive.")
    _bounds_sizes(policy, betas, n_lower, n_outer, n_inner)
    _validate(S0, K, T, r, sigma, n_paths, n_steps, option_type, need_sigma=(model_l == "gbm"))
    _betas_shape(betas, n_steps, 4)
    _bounds_scheme("barrier", model_l, heston_scheme)
    up = barrier_type.startswith("up")
    if (float(S0) >= H) if up else (float(S0) <= H):
        raise ValueError("S0 lies on or beyond the barrier (the option is already knocked).")
    M = _even_paths(n_paths)
    p = _law_params(model_l, option_type, heston_scheme, heston_params, M, n_steps, S0, K, r, sigma, T, seed, stream)
    c = ctx or _ffi.default_context(device)
    out = c.price_barrier_bounds(p, barrier_type, H, policy=policy, n_lower=int(n_lower), n_outer=int(n_outer),
                                 n_inner=int(n_inner), betas=betas, exercise_every=every,
                                 suboptimality_check=suboptimality_check)
    return _bounds_result(BarrierBoundsResult, out, policy=policy, option_type=option_type, **_game(n_steps, every),
                          suboptimality_check=suboptimality_check or "off", barrier=H, barrier_type=barrier_type,
                          monitoring="discrete", model=model_l)


def price_bermudan_bounds(S0, K, r, sigma, T, n_paths, n_steps, exercise_every, model="GBM", option_type="put",
                          policy="textbook", n_lower=1_000_000, n_outer=8192, n_inner=1024, heston_params=None,
                          heston_scheme="reference", seed=42, stream=0, betas=None, device=None, ctx=None,
                          control_variate=False) -> BoundsResult:
    """Lower and upper bounds on the value of a Bermudan option that may be exercised at every exercise_every-th date of a
    grid of n_steps dates, counted back from expiry, and at expiry: price_american_bounds (model
    "GBM") or price_american_bounds_heston (model "Heston", a policy on the spot; sigma only sets the defaults of
    heston_defaults) with that schedule.  0 or 1 is the game on every date, exercise_every >= n_steps the European option.
    The bracket for the quote of price_bermudan_option, which is a two-pass-flow value and lies above `upper`.
    control_variate=True: as price_american_bounds takes it, model "GBM" only."""
    if exercise_every is None or isinstance(exercise_every, (list, tuple)):
        raise ValueError("exercise_every must be a non-negative integer.")
    model_l = str(model).lower()
    _true_or_false(control_variate)
    if control_variate and model_l == "heston":
        raise ValueError("control_variate: the Black-Scholes control variate is for model 'GBM' only.")
    if model_l == "gbm":
        return price_american_bounds(S0, K, r, sigma, T, n_paths, n_steps, option_type=option_type, policy=policy,
                                     n_lower=n_lower, n_outer=n_outer, n_inner=n_inner, seed=seed, stream=stream, betas=betas,
                                     device=device, ctx=ctx, control_variate=control_variate,
                                     exercise_every=exercise_every)
    if model_l == "heston":
        return price_american_bounds_heston(S0, K, r, T, n_paths, n_steps, heston_params=heston_defaults(sigma, heston_params),
                                            heston_scheme=heston_scheme, option_type=option_type, policy=policy,
                                            n_lower=n_lower, n_outer=n_outer, n_inner=n_inner, seed=seed, stream=stream,
                                            betas=betas, device=device, ctx=ctx, exercise_every=exercise_every)
    raise ValueError("model must be 'GBM' or 'Heston'.")


def price_american_bounds_checked(S0, K, r, sigma, T, n_paths, n_steps, check="european", model="GBM", option_type="put",
                                  policy="textbook", n_lower=1_000_000, n_outer=8192, n_inner=1024, heston_params=None,
                                  heston_scheme="reference", seed=42, stream=0, betas=None, device=None, ctx=None,
                                  control_variate=False, exercise_every=0) -> BoundsResult:
    """price_american_bounds (model "GBM") or price_american_bounds_heston (model "Heston", a policy on the spot; sigma only
    sets the defaults of heston_defaults) with Broadie-Cao's sub-optimality checking: the inner
    simulations run only at the (outer path, date) items at which exercise is not known to be sub-optimal, and the walk
    visits only those dates.  check="payoff" keeps an item when the option is in the money there, "european" (GBM only) when
    the payoff exceeds the Black-Scholes value of the European option; date 0 and every date at which the policy stops are
    always kept, "off" keeps everything.  The paths, the stops, the policy and `lower` are the unchecked call's; `upper`
    stays an upper bound and is at most the unchecked one up to rounding; `inner_path_steps` counts the work that was done.
    control_variate=True: as price_american_bounds takes it, model "GBM" only.  The game is the one on every date:
    exercise_every must be 0 or 1."""
    if check not in _ffi.BOUND_CHECKS:
        raise ValueError(f"check must be one of {list(_ffi.BOUND_CHECKS)}.")
    if _one_schedule(exercise_every) >= 2:
        raise ValueError("sub-optimality checking is for the game on every date (exercise_every must be 0 or 1).")
    model_l = _model_name(model)
    _true_or_false(control_variate)
    if model_l == "heston" and control_variate:
        raise ValueError("control_variate: the Black-Scholes control variate is for model 'GBM' only.")
    if model_l == "heston" and check == "european":
        raise ValueError("check='european' is for model 'GBM' only (model 'Heston' takes 'payoff' or 'off').")
    c = ctx or _ffi.default_context(device)
    with c._bounds_checking(check):
        if model_l == "gbm":
            res = price_american_bounds(S0, K, r, sigma, T, n_paths, n_steps, option_type=option_type, policy=policy,
                                        n_lower=n_lower, n_outer=n_outer, n_inner=n_inner, seed=seed, stream=stream,
                                        betas=betas, ctx=c, control_variate=control_variate, exercise_every=0)
        else:
            res = price_american_bounds_heston(S0, K, r, T, n_paths, n_steps,
                                               heston_params=heston_defaults(sigma, heston_params),
                                               heston_scheme=heston_scheme, option_type=option_type, policy=policy,
                                               n_lower=n_lower, n_outer=n_outer, n_inner=n_inner, seed=seed, stream=stream,
                                               betas=betas, ctx=c, exercise_every=0)
    res.suboptimality_check = check
    return res


@dataclass
class BasketBoundsResult(BoundsResult):
    """price_american_basket_bounds: BoundsResult for the index of a basket, with the index of the initial spots, the number
    of assets and the kind.  With regressors "index" the policy is a function of the index alone, with "index+runner-up" of
    the index and the second order statistic of the weighted spots (`betas` is then [n_steps+1][8] = c0 .. c5, n, 0);
    `lower` is what that policy earns, `upper` bounds the value of the multi-asset game under ANY policy."""
    index0: float = 0.0
    n_assets: int = 1
    kind: str = "basket"
    regressors: str = "index"


def price_american_basket_bounds(spots, K, r, sigmas, T, n_paths, n_steps, correlation=None, weights=None,
                                 dividend_yields=None, kind="basket", option_type="put", policy="textbook",
                                 n_lower=1_000_000, n_outer=8192, n_inner=1024, seed=42, stream=0, betas=None, device=None,
                                 ctx=None, regressors="index", suboptimality_check=None) -> BasketBoundsResult:
    """Lower and upper bounds on the Bermudan value of an option on an index of 1 .. 8 correlated GBM assets
    (omc_price_american_basket_bounds): price_american_bounds with the assets, kinds and defaults of
    price_american_basket.  The policy (`policy` / `betas` as price_american_bounds takes them) regresses on the index
    alone; the lower-bound, outer and inner paths use Philox streams stream + 1, + 2, + 3.  With one asset and a dividend
    yield these are the bounds of a single stock with a continuous yield.  kind="geometric": the geometric index is itself
    one GBM, so the call is made with ONE asset (G0, sigma_G, q_G) of weight 1 -- n_assets of the result is then 1 and
    index0 is G0.  One GPU.
    regressors="index+runner-up" (DESIGN.md section 18): for kind "best-of" / "worst-of" on 2 .. 8 assets the policy also
    sees the runner-up, the second largest (smallest) weighted spot -- on the two-asset max-call benchmark that closes nine
    tenths of the gap between the index policy's lower bound and the lattice value.  policy is then "textbook" or "given",
    and `betas` is [n_steps+1][8] = c0, c1, c2 (1, u, u^2 of the index), c3, c4 (w, w^2 of the runner-up), c5 (u w), n, 0.
    kind "asian" / "asian-geometric" (DESIGN.md section 23): the index is the running average; the inner paths start at the
    outer path's asset spots and running sum.  regressors="index+spot" is theirs alone: the policy also sees the current
    basket value, the other half of the Markov state (average, spot), with the table and the policies of
    "index+runner-up"; at most 512 steps.
    suboptimality_check="payoff" (regressors "index" only): inner simulations only at the items at
    which the index is in the money or the policy stops, and at date 0; "off" or None: every item."""
    if suboptimality_check is not None and suboptimality_check not in _ffi.BOUND_CHECKS:
        raise ValueError(f"suboptimality_check must be one of {list(_ffi.BOUND_CHECKS)} or None.")
    if suboptimality_check == "european":
        raise ValueError("suboptimality_check='european' is for one GBM asset (price_american_bounds_checked).")
    if suboptimality_check == "payoff" and regressors != "index":
        raise ValueError("suboptimality_check='payoff' is for regressors='index'.")
    _bounds_sizes(policy, betas, n_lower, n_outer, n_inner)
    S0, sig, q, w, rho = _basket_args(spots, sigmas, weights, dividend_yields, correlation, kind)
    _ffi.check_runnerup(regressors, policy, kind, len(S0))
    if regressors == "index+spot" and int(n_steps) > _ffi.HESTON_SV_MAX_STEPS:
        raise ValueError(f"regressors='index+spot' takes at most {_ffi.HESTON_SV_MAX_STEPS} steps.")
    _validate(S0[0], K, T, r, sig[0], n_paths, n_steps, option_type)
    M = _even_paths(n_paths)
    p = _ffi.make_params(model="gbm", is_put=(option_type == "put"), semantics="two_pass", antithetic=True, n_paths=M,
                         n_steps=int(n_steps), S0=S0[0], K=K, r=r, sigma=sig[0], T=T, seed=seed, stream=stream)
    b = _ffi.make_basket(S0, sig, q, w, rho, kind)
    if kind == "geometric":  # one GBM: (G0, sigma_G, q_G) of the library's own table
        G0, sigma_G, q_G = _ffi.basket_table(p, b)[4]
        b = _ffi.make_basket([G0], [sigma_G], [q_G], [1.0], None, "basket")
    c = ctx or _ffi.default_context(device)
    out = c.price_american_basket_bounds(p, b, policy=policy, n_lower=int(n_lower), n_outer=int(n_outer),
                                         n_inner=int(n_inner), betas=betas, regressors=regressors,
                                         suboptimality_check=suboptimality_check)
    return _bounds_result(BasketBoundsResult, out, policy=policy, option_type=option_type, index0=out["index0"],
                          n_assets=out["n_assets"], kind=kind, regressors=regressors,
                          suboptimality_check=suboptimality_check or "off")


_ASIAN_AVERAGING = {"arithmetic": "asian", "geometric": "asian-geometric"}


def price_asian_option(S0, K, r, sigma, T, n_paths, n_steps, option_type="put", averaging="arithmetic", dividend_yield=0.0,
                       bounds=False, seed=None, device=None, **bounds_args):
    """Fixed-strike average-price (Asian) option with early exercise on one GBM stock: the one-asset
    call of price_american_basket with kind "asian" (averaging="arithmetic") or "asian-geometric" ("geometric") and weight
    1.  The average runs over the grid dates 1 .. t; S0 is not in it.  bounds=False -> BasketResult, the two-pass price.
    bounds=True -> BasketBoundsResult of price_american_basket_bounds, which takes the further keywords (policy, n_lower,
    n_outer, n_inner, stream, betas, ctx, regressors="index" | "index+spot")."""
    if averaging not in _ASIAN_AVERAGING:
        raise ValueError(f"averaging must be one of {list(_ASIAN_AVERAGING)}.")
    kind = _ASIAN_AVERAGING[averaging]
    common = dict(weights=[1.0], dividend_yields=[float(dividend_yield)], kind=kind, option_type=option_type, device=device)
    if not bounds:
        if bounds_args:
            raise ValueError(f"{sorted(bounds_args)} are arguments of the bounds (bounds=True).")
        return price_american_basket([S0], K, r, [sigma], T, n_paths, n_steps, seed=seed, **common)
    return price_american_basket_bounds([S0], K, r, [sigma], T, n_paths, n_steps, seed=42 if seed is None else seed,
                                        **common, **bounds_args)


_job = {}


def _in_job(n_gpus: int) -> bool:
    """Is this process one rank of an n_gpus-rank job (started by a launcher that set the rank environment)?
    A job of ANOTHER size is an error, not a reason to start ranks from inside a rank."""
    if "RANK" not in os.environ:
        return False
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == n_gpus:
        return True
    if world > 1:
        raise RuntimeError(
            f"price_american_option(n_gpus={n_gpus}) was called inside a {world}-rank job (RANK="
            f"{os.environ['RANK']}): n_gpus must equal the job's WORLD_SIZE.  It does not fall back to one GPU.")
    return False


def _job_pricer(n_gpus: int, device=None):
    """The per-process RcclPricer of an n_gpus-rank job (created on first use, closed at exit)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != n_gpus or "RANK" not in os.environ:
        raise RuntimeError(
            f"this process is not a rank of a {n_gpus}-rank job (WORLD_SIZE={os.environ.get('WORLD_SIZE', 'unset')}, "
            f"RANK={os.environ.get('RANK', 'unset')}); it does not fall back to one GPU.")
    key = (os.getpid(), n_gpus)
    sp = _job.get(key)
    if sp is None:
        import atexit

        from .dist import RcclPricer
        rank = int(os.environ["RANK"])
        if isinstance(device, (list, tuple)):  # one device per rank
            device = device[rank]
        local = int(os.environ.get("LOCAL_RANK", rank)) if device is None else int(device)
        sp = RcclPricer(local, rank, world)
        _job[key] = sp
        atexit.register(sp.close)
    return sp


def price_european_option(S0, K, r, sigma, T, n_paths, n_steps=1, model="GBM", option_type="put",
                          heston_params=None, heston_scheme="reference", antithetic=True, seed=42,
                          stream=0, device=0, ctx=None) -> PriceResult:
    """Discounted terminal payoff mean; no path matrix is stored (options_model_3.py:382-437)."""
    model_l = str(model).lower()
    _validate(S0, K, T, r, sigma, n_paths, n_steps, option_type, need_sigma=(model_l == "gbm"))
    _validate_scheme(model_l, heston_scheme, sigma, heston_params)
    M = int(n_paths) // 2 * 2 if antithetic else int(n_paths)
    hp = heston_defaults(sigma, heston_params)
    c = ctx or _ffi.default_context(device)
    p = _ffi.make_params(model=model_l, is_put=(option_type == "put"), antithetic=antithetic,
                         heston_scheme=heston_scheme, n_paths=M, n_steps=int(n_steps), S0=S0, K=K,
                         r=r, sigma=sigma or 0.0, T=T, seed=seed, stream=stream, **hp)
    out = c.price_european(p)
    var = max(out["sumsq"] / M - out["price"] ** 2, 0.0)
    return PriceResult(price=out["price"], stderr=math.sqrt(var / max(M - 1, 1)), std=out["std"],
                       zero_prob=out["zero_prob"], n_paths=M, n_exercised=0, sum_nitm=0,
                       model=model_l, semantics="european", option_type=option_type,
                       timings_ms=dict(total=out["ms_total"]))
