"""ctypes binding of libomc.so (include/omc.h).  No torch, no numpy compute: this module
only marshals arguments.  If the HIP library is missing or there is no GPU the calls fail
loudly -- there is no CPU fallback in the product path.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import threading

import numpy as np

from . import _build

ABI_VERSION = 14

SEMANTICS = {"reference": 0, "textbook": 1, "two_pass": 2}
MODELS = {"gbm": 0, "heston": 1}
HESTON_SCHEMES = {"reference": 0, "clamp": 0, "full_truncation": 1, "calibrator": 2, "qe": 3}
BARRIER_KINDS = {"down-and-out": 0, "up-and-out": 1, "down-and-in": 2, "up-and-in": 3}
MONITORING = {"discrete": 0, "continuous": 1}
DIVIDEND_KINDS = {"proportional": 0, "cash": 1}
# argument errors of the dividend entry points (include/omc.h): raised as DividendError
DIVIDEND_ERRORS = range(-24, -16)
BASKET_KINDS = {"basket": 0, "arithmetic": 0, "geometric": 1, "best-of": 2, "worst-of": 3, "asian": 5,
                "asian-geometric": 6}
BASKET_MAX_ASSETS = 8
BOUND_POLICIES = {"reference": 0, "textbook": 1, "two_pass": 2, "given": 3}
BOUND_REGRESSORS = ("index", "index+runner-up", "index+spot")  # what the policy of the multi-asset bounds sees
ASIAN_KINDS = (5, 6)  # the running-average kinds: "index+spot" is theirs, "index+runner-up" best-of's and worst-of's
HESTON_BOUND_REGRESSORS = ("spot", "spot+variance")  # ... of the Heston bounds: the codes of omc_bounds_config.regressors
HESTON_SV_MAX_STEPS = 512  # dates of a spot+variance policy (its rows live in LDS)
BOUND_CHECKS = ("off", "payoff", "european")  # sub-optimality checking: the codes of option "bounds_suboptimality"


def check_runnerup(regressors, policy, kind, n_assets):
    """The argument checks of regressors="index+runner-up" (omc_price_american_basket_bounds_runnerup), raised as
    ValueError before anything touches the device.  kind: a key of BASKET_KINDS or its code."""
    if regressors not in BOUND_REGRESSORS:
        raise ValueError(f"regressors must be one of {list(BOUND_REGRESSORS)}.")
    if regressors == "index":
        return
    if BOUND_POLICIES.get(policy, policy) not in (BOUND_POLICIES["textbook"], BOUND_POLICIES["given"]):
        raise ValueError(f"regressors='{regressors}' takes policy 'textbook' or 'given'.")
    if regressors == "index+spot":  # the average and the current basket value
        if BASKET_KINDS.get(kind, kind) not in ASIAN_KINDS:
            raise ValueError("regressors='index+spot' is for kind 'asian' or 'asian-geometric'.")
        return
    if BASKET_KINDS.get(kind, kind) not in (BASKET_KINDS["best-of"], BASKET_KINDS["worst-of"]):
        raise ValueError("regressors='index+runner-up' is for kind 'best-of' or 'worst-of'.")
    if int(n_assets) < 2:
        raise ValueError("regressors='index+runner-up' needs at least two assets.")


def heston_regressors_code(regressors):
    """a key of HESTON_BOUND_REGRESSORS -> its code, omc_bounds_config.regressors (ValueError for anything else)"""
    if regressors not in HESTON_BOUND_REGRESSORS:
        raise ValueError(f"regressors must be one of {list(HESTON_BOUND_REGRESSORS)}.")
    return HESTON_BOUND_REGRESSORS.index(regressors)


def check_heston_regressors(regressors, policy, n_steps, v0, theta):
    """The argument checks of regressors="spot+variance" (omc_price_american_bounds_heston with cfg.regressors = 1), raised
    as ValueError before anything touches the device."""
    if heston_regressors_code(regressors) == 0:
        return
    if BOUND_POLICIES.get(policy, policy) not in (BOUND_POLICIES["textbook"], BOUND_POLICIES["given"]):
        raise ValueError("regressors='spot+variance' takes policy 'textbook' or 'given'.")
    if int(n_steps) > HESTON_SV_MAX_STEPS:
        raise ValueError(f"regressors='spot+variance' takes at most {HESTON_SV_MAX_STEPS} steps.")
    if not max(float(v0), float(theta)) > 0.0:
        raise ValueError("regressors='spot+variance' scales the variance by max(v0, theta), which must be positive.")


class OmcError(RuntimeError):
    pass


class DividendError(OmcError, ValueError):
    """An argument of the dividend entry points the library refuses (codes -17 .. -24 of include/omc.h)."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class Params(C.Structure):
    _fields_ = [("model", C.c_int32), ("is_put", C.c_int32), ("semantics", C.c_int32),
                ("antithetic", C.c_int32), ("heston_scheme", C.c_int32), ("n_steps", C.c_int32),
                ("n_paths", C.c_int64),
                ("S0", C.c_double), ("K", C.c_double), ("r", C.c_double), ("sigma", C.c_double),
                ("T", C.c_double),
                ("v0", C.c_double), ("kappa", C.c_double), ("theta", C.c_double), ("xi", C.c_double),
                ("rho", C.c_double),
                ("seed", C.c_uint64), ("stream", C.c_uint64), ("pair_offset", C.c_uint64)]


class Result(C.Structure):
    _fields_ = [("price", C.c_double), ("sum", C.c_double), ("sumsq", C.c_double),
                ("std", C.c_double), ("zero_prob", C.c_double),
                ("n_paths", C.c_int64), ("n_exercised", C.c_int64), ("n_zero", C.c_int64),
                ("sum_nitm", C.c_int64),
                ("ms_paths", C.c_double), ("ms_lsm", C.c_double), ("ms_total", C.c_double),
                ("ms_pass1", C.c_double), ("ms_pass2", C.c_double), ("timed", C.c_int64),
                ("folded", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def _with_base(out):
    """A result struct that extends omc_result as one dict: the base pricing's keys plus its own fields."""
    d = out.base.as_dict()
    d.update({k: getattr(out, k) for k, _ in out._fields_ if k not in ("base", "reserved")})
    return d


class Greeks(C.Structure):
    """omc_greeks: the base pricing plus the frozen-policy pathwise Greeks (omc_price_american_greeks)."""
    _fields_ = [("base", Result),
                ("delta", C.c_double), ("gamma", C.c_double), ("vega", C.c_double), ("rho", C.c_double),
                ("theta", C.c_double),
                ("se_delta", C.c_double), ("se_gamma", C.c_double), ("se_vega", C.c_double), ("se_rho", C.c_double),
                ("se_theta", C.c_double),
                ("bump", C.c_double), ("price_up", C.c_double), ("price_down", C.c_double),
                ("n_exercised_up", C.c_int64), ("n_exercised_down", C.c_int64),
                ("ms_greeks", C.c_double)]


class Barrier(C.Structure):
    """omc_barrier: kind (BARRIER_KINDS), monitoring (MONITORING), american (1 / 0), H."""
    _fields_ = [("kind", C.c_int32), ("monitoring", C.c_int32), ("american", C.c_int32), ("reserved", C.c_int32),
                ("H", C.c_double)]


class BarrierResult(C.Structure):
    """omc_barrier_result: the American pricing of the encoded matrix plus the European knock-out / knock-in sums."""
    _fields_ = [("base", Result),
                ("euro_out", C.c_double), ("euro_out_se", C.c_double), ("euro_in", C.c_double),
                ("euro_in_se", C.c_double), ("hit_prob", C.c_double), ("ms_barrier_paths", C.c_double)]


class Dividend(C.Structure):
    """omc_dividend: ex-dividend time t in (0, T], amount (delta or currency units), kind (DIVIDEND_KINDS)."""
    _fields_ = [("t", C.c_double), ("amount", C.c_double), ("kind", C.c_int32), ("reserved", C.c_int32)]


class DivResult(C.Structure):
    """omc_div_result: the pricing plus the generator's time and the dividend steps of the schedule."""
    _fields_ = [("base", Result), ("ms_div_paths", C.c_double), ("n_div_steps", C.c_int32),
                ("first_div_step", C.c_int32)]


class DivGreeks(C.Structure):
    """omc_div_greeks (include/omc_dividend_greeks.h): omc_greeks plus epsilon (dV/dq) and the dividend steps."""
    _fields_ = [("g", Greeks), ("epsilon", C.c_double), ("se_epsilon", C.c_double), ("n_div_steps", C.c_int32),
                ("first_div_step", C.c_int32)]


class Jump(C.Structure):
    """omc_jump: lambda (jumps per year), mu_j and sigma_j (mean and standard deviation of a jump's log size)."""
    _fields_ = [("lambda_", C.c_double), ("mu_j", C.c_double), ("sigma_j", C.c_double)]


class JumpResult(C.Structure):
    """omc_jump_result: the pricing plus the generator's time, the compensator, the drift rate and the largest count."""
    _fields_ = [("base", Result), ("ms_jump_paths", C.c_double), ("kappa", C.c_double), ("drift_rate", C.c_double),
                ("n_thresholds", C.c_int32), ("reserved", C.c_int32)]


class JumpGreeks(C.Structure):
    """omc_jump_greeks (include/omc_jump_greeks.h): omc_greeks plus epsilon (dV/dq), the jump Greeks and the jump count."""
    _fields_ = [("g", Greeks), ("epsilon", C.c_double), ("se_epsilon", C.c_double),
                ("dlambda", C.c_double), ("se_dlambda", C.c_double), ("dmu_j", C.c_double), ("se_dmu_j", C.c_double),
                ("dsigma_j", C.c_double), ("se_dsigma_j", C.c_double),
                ("theta_score", C.c_double), ("se_theta_score", C.c_double),
                ("kappa", C.c_double), ("drift_rate", C.c_double), ("n_jumps", C.c_int64)]


class Basket(C.Structure):
    """omc_basket: n_assets (1 .. 8), kind (BASKET_KINDS), per-asset S0 / sigma / q / w, and rho row-major [d][d]."""
    _fields_ = [("n_assets", C.c_int32), ("kind", C.c_int32), ("S0", C.c_double * 8), ("sigma", C.c_double * 8),
                ("q", C.c_double * 8), ("w", C.c_double * 8), ("rho", C.c_double * 64)]


class BasketResult(C.Structure):
    """omc_basket_result: the pricing of the index matrix plus the generator's time and the index of the initial spots."""
    _fields_ = [("base", Result), ("ms_basket_paths", C.c_double), ("index0", C.c_double), ("n_assets", C.c_int32),
                ("kind", C.c_int32)]


class BasketGreeks(C.Structure):
    """omc_basket_greeks: the base pricing plus the frozen-policy per-asset Greeks (omc_price_american_basket_greeks)."""
    _fields_ = [("base", BasketResult),
                ("delta", C.c_double * 8), ("gamma", C.c_double * 8), ("vega", C.c_double * 8),
                ("se_delta", C.c_double * 8), ("se_gamma", C.c_double * 8), ("se_vega", C.c_double * 8),
                ("rho", C.c_double), ("theta", C.c_double), ("se_rho", C.c_double), ("se_theta", C.c_double),
                ("bump", C.c_double), ("price_up", C.c_double * 8), ("price_down", C.c_double * 8),
                ("n_exercised_up", C.c_int64 * 8), ("n_exercised_down", C.c_int64 * 8),
                ("ms_greeks", C.c_double), ("gamma_on", C.c_int32), ("reserved", C.c_int32)]


class BoundsConfig(C.Structure):
    """omc_bounds_config: policy (BOUND_POLICIES), the three sizes and the three Philox streams."""
    _fields_ = [("policy", C.c_int32), ("regressors", C.c_int32), ("n_lower", C.c_int64), ("n_outer", C.c_int64),
                ("n_inner", C.c_int64), ("stream_lower", C.c_uint64), ("stream_outer", C.c_uint64),
                ("stream_inner", C.c_uint64)]


class Bounds(C.Structure):
    """omc_bounds: the Andersen-Broadie lower / upper bounds of the Bermudan game on the grid (omc_price_american_bounds)."""
    _fields_ = [("lower", C.c_double), ("se_lower", C.c_double), ("upper", C.c_double), ("se_upper", C.c_double),
                ("ci_lo", C.c_double), ("ci_hi", C.c_double),
                ("n_lower", C.c_int64), ("n_outer", C.c_int64), ("n_inner", C.c_int64), ("n_exercised_lower", C.c_int64),
                ("inner_path_steps", C.c_int64),
                ("ms_fit", C.c_double), ("ms_lower", C.c_double), ("ms_upper", C.c_double), ("ms_total", C.c_double)]


class BasketBounds(C.Structure):
    """omc_basket_bounds: omc_bounds of the index of a basket plus the index of the initial spots, n_assets and kind."""
    _fields_ = [("bounds", Bounds), ("index0", C.c_double), ("n_assets", C.c_int32), ("kind", C.c_int32)]


class ChainEntry(C.Structure):
    """omc_chain_entry: strike, side and exercise schedule of one quote of a chain (omc_price_american_chain);
    exercise_every 0 or 1 = every date (American), k >= 2 = every k-th date counted back from expiry (Bermudan)."""
    _fields_ = [("K", C.c_double), ("is_put", C.c_int32), ("exercise_every", C.c_int32)]


class ChainInfo(C.Structure):
    """omc_chain_info: storage and route of a chain, its sweep launches per pass and its phase times."""
    _fields_ = [("folded", C.c_int32), ("fused", C.c_int32), ("n_launch_groups", C.c_int32), ("reserved", C.c_int32),
                ("ms_paths", C.c_double), ("ms_pass1", C.c_double), ("ms_pass2", C.c_double), ("ms_total", C.c_double)]


CHAIN_MAX = 256
CHAIN_BOUNDS_MAX = 8  # OMC_CHAIN_BOUNDS_MAX: entries of a chain of price bounds that ride on one simulation at most


class ChainBoundsInfo(C.Structure):
    """omc_chain_bounds_info: the steps the chain's inner pairs were simulated for, its groups and its phase times."""
    _fields_ = [("inner_path_steps_simulated", C.c_int64), ("n_groups", C.c_int32), ("entries_per_group", C.c_int32),
                ("ms_fit", C.c_double), ("ms_lower", C.c_double), ("ms_upper", C.c_double), ("ms_total", C.c_double)]


class ChainGreeksInfo(C.Structure):
    """omc_chain_greeks_info: storage, groups and sweep launches of a chain's Greeks and its phase times."""
    _fields_ = [("folded", C.c_int32), ("n_groups", C.c_int32), ("n_sweep_launches", C.c_int32),
                ("entries_per_launch", C.c_int32),
                ("ms_paths", C.c_double), ("ms_pass1", C.c_double), ("ms_greeks", C.c_double), ("ms_total", C.c_double)]


class MlpJob(C.Structure):
    """omc_mlp_job: one network of a batch trained side by side (omc_mlp_train_epoch_batch)."""
    _fields_ = [("data", C.c_void_p), ("n_rows", C.c_int64), ("batch", C.c_int64),
                ("params", C.c_void_p), ("adam_m", C.c_void_p), ("adam_v", C.c_void_p),
                ("step", C.c_int64), ("lr", C.c_double), ("seed", C.c_uint64), ("shuffle_key", C.c_uint64),
                ("mean_loss", C.c_double)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)

# name -> (restype, argtypes); every symbol include/omc.h declares
_P, _I, _I64, _U64, _D, _SZ = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_double, C.c_size_t
SIGNATURES = {
    "omc_abi_version": (C.c_int, []),
    "omc_last_error": (C.c_char_p, []),
    "omc_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "omc_ctx_create": (C.c_int, [_I, _P, C.POINTER(_P)]),
    "omc_ctx_destroy": (C.c_int, [_P]),
    "omc_sync": (C.c_int, [_P]),
    "omc_alloc": (C.c_int, [_P, _SZ, C.POINTER(_P)]),
    "omc_free": (C.c_int, [_P, _P]),
    "omc_memcpy_h2d": (C.c_int, [_P, _P, _P, _SZ]),
    "omc_memcpy_d2h": (C.c_int, [_P, _P, _P, _SZ]),
    "omc_set_option": (C.c_int, [_P, C.c_char_p, _I64]),
    "omc_gbm_paths_f32": (C.c_int, [_P, _P, _I64, _I64, _I, _D, _D, _D, _D, _U64, _U64, _U64, _I]),
    "omc_heston_paths_f32": (C.c_int, [_P, _P, _I64, _I64, _I] + [_D] * 8 + [_U64, _U64, _U64, _I]),
    "omc_heston_paths_sv_f32": (C.c_int, [_P, _P, _P, _I64, _I64, _I] + [_D] * 8 + [_U64, _U64, _U64, _I]),
    "omc_gbm_paths_from_normals_f32": (C.c_int, [_P, _P, _I64, _I64, _I, _D, _D, _D, _D, _P, _I64, _I]),
    "omc_heston_paths_from_normals_f32": (C.c_int, [_P, _P, _I64, _I64, _I] + [_D] * 8 + [_P, _P, _I64, _I]),
    "omc_philox4x32_10": (C.c_int, [_P, _P, _P, _I]),
    "omc_gbm_normals_f32": (C.c_int, [_P, _P, _I64, _I64, _I, _U64, _U64, _U64]),
    "omc_lsm_poly": (C.c_int, [_P, _P, _I64, _I64, _I, _D, _D, _D, _I, _I, C.POINTER(Result), _P, _P, _P]),
    "omc_lsm_apply_frozen": (C.c_int, [_P, _P, _I64, _I64, _I, _D, _D, _D, _I, _P, C.POINTER(Result), _P, _P]),
    "omc_lsm_apply_values": (C.c_int, [_P, _P, _I64, _I64, _I, _D, _D, _D, _I, _I, _P, _I64, C.POINTER(Result), _P, _P]),
    "omc_lsm_contnet": (C.c_int, [_P, _P, _I64, _I64, _I, _D, _D, _D, _I, _I, _I, _D, _U64, C.POINTER(Result), _P, _P]),
    "omc_price_american_contnet": (C.c_int, [_P, C.POINTER(Params), _I, _I, _D, _U64, C.POINTER(Result)]),
    "omc_contnet_init_params": (C.c_int, [_P, _I, _I, _U64, _P, _I]),
    "omc_set_allreduce_hook": (C.c_int, [_P, ALLREDUCE_FN, _P]),
    "omc_comm_unique_id": (C.c_int, [_P, _SZ]),
    "omc_comm_init": (C.c_int, [_P, _I, _I, _P, _SZ]),
    "omc_comm_destroy": (C.c_int, [_P]),
    "omc_comm_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "omc_comm_allreduce_f64": (C.c_int, [_P, _P, _I, _I]),
    "omc_p2p_export": (C.c_int, [_P, _P, _SZ]),
    "omc_p2p_connect": (C.c_int, [_P, _I, _I, _P, _SZ]),
    "omc_p2p_disconnect": (C.c_int, [_P]),
    "omc_p2p_status": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "omc_price_american": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Result), _P, _I64]),
    "omc_price_american_greeks": (C.c_int, [_P, C.POINTER(Params), _D, _P, _P, C.POINTER(Greeks)]),
    "omc_pass2_tables_check": (C.c_int, [_P, _I, _D, _I, _P, _P, _I, _P, _P]),
    "omc_price_european": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Result)]),
    "omc_price_barrier": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Barrier), C.POINTER(BarrierResult), _P, _I64]),
    "omc_dividend_schedule": (C.c_int, [C.POINTER(Params), _D, C.POINTER(Dividend), _I, _P, _P, _P]),
    "omc_price_american_div": (C.c_int, [_P, C.POINTER(Params), _D, C.POINTER(Dividend), _I, C.POINTER(DivResult), _P,
                                         _I64]),
    "omc_jump_table": (C.c_int, [C.POINTER(Params), C.POINTER(Jump), _D, _P, C.POINTER(_D), C.POINTER(_D)]),
    "omc_price_american_jump": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Jump), _D, C.POINTER(JumpResult), _P, _I64]),
    "omc_basket_table": (C.c_int, [C.POINTER(Params), C.POINTER(Basket), _P, _P, _P, C.POINTER(_D), _P]),
    "omc_price_american_basket": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Basket), C.POINTER(BasketResult), _P, _P,
                                            _I64]),
    "omc_price_american_basket_greeks": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Basket), _D, _I, _P, _P,
                                                   C.POINTER(BasketGreeks)]),
    "omc_price_american_bounds": (C.c_int, [_P, C.POINTER(Params), C.POINTER(BoundsConfig), _P, _P, _P, _P,
                                            C.POINTER(Bounds)]),
    "omc_price_american_basket_bounds": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Basket), C.POINTER(BoundsConfig), _P,
                                                   _P, _P, _P, C.POINTER(BasketBounds)]),
    "omc_price_american_basket_bounds_runnerup": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Basket),
                                                            C.POINTER(BoundsConfig), _P, _P, _P, _P,
                                                            C.POINTER(BasketBounds)]),
    "omc_price_american_bounds_heston": (C.c_int, [_P, C.POINTER(Params), C.POINTER(BoundsConfig), _P, _P, _P, _P,
                                                   C.POINTER(Bounds)]),
    "omc_heston_price_strikes": (C.c_int, [_P, _I64, _I] + [_D] * 8 + [_U64, _U64, _I, _P, _I, _I, _P, _P]),
    "omc_heston_price_surface": (C.c_int, [_P, _I64, _I] + [_D] * 7 + [_U64, _I, _P, _P, _I, _P, _P, _I, _I, _P, _P]),
    "omc_price_american_seq": (C.c_int, [_P, C.POINTER(Params), _I, C.POINTER(Result)]),
    "omc_seq_step_width": (C.c_int, [_P, C.POINTER(Params), _I]),
    "omc_seq_group_width": (C.c_int, [_P, C.POINTER(Params), _I]),
    "omc_price_american_chain": (C.c_int, [_P, C.POINTER(Params), C.POINTER(ChainEntry), _I, C.POINTER(Result), _P,
                                           C.POINTER(ChainInfo)]),
    "omc_chain_width": (C.c_int, [_P, C.POINTER(Params), _I]),
    "omc_price_american_batch": (C.c_int, [_P, C.POINTER(Params), _I, C.POINTER(Result)]),
    "omc_price_european_batch": (C.c_int, [_P, C.POINTER(Params), _I, C.POINTER(Result)]),
    "omc_price_american_contnet_batch": (C.c_int, [_P, C.POINTER(Params), _I, _I, _I, _D, C.POINTER(C.c_uint64),
                                                   C.POINTER(Result)]),
    "omc_mlp_param_count": (C.c_int, [_I, _I]),
    "omc_mlp_train_supported": (C.c_int, [_I, _I, _I64]),
    "omc_mlp_train_epoch": (C.c_int, [_P, _P, _I64, _I64, _I, _I, _P, _P, _P, C.POINTER(C.c_int64)]
                            + [_D] * 6 + [_U64, _U64, C.POINTER(C.c_double)]),
    "omc_mlp_train_batch_supported": (C.c_int, [_I, _I, _I64]),
    "omc_mlp_train_epoch_batch": (C.c_int, [_P, C.POINTER(MlpJob), _I, _I, _I] + [_D] * 5),
    "omc_mlp_shuffle_indices": (C.c_int, [_P, _I64, _U64, _P]),
    "omc_mlp_train_variant": (C.c_int, [C.c_int, C.c_int, _I64]),
    "omc_price_american_ols7": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Result), _P, _P]),
    "omc_lsm_ols7": (C.c_int, [_P, _P, _I64, _I64, _I, _D, _D, _D, _I, C.POINTER(Result), _P, _P, _P, _P]),
    "omc_ctx_device_info": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int]),
    "omc_mlp_dropout_masks": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _I64, _P, C.c_uint32, _U64, C.c_double, _P]),
    "omc_nn_half_counts": (C.c_int, [_P, _P, _I64, _I64, _I, _D, _I, _P]),
    "omc_mlp_shard_epoch": (C.c_int, [_P, _P, _I64, _I64, _I64, _U64, _P, _P, _I, _I, _P, _P, _P]),
    "omc_mlp_train_epoch_sharded": (C.c_int, [_P, _P, _I64, _I64, _I64, _I, _I, _P, _P, _P, C.POINTER(C.c_int64)]
                                    + [_D] * 6 + [_U64, _P, _P, C.POINTER(C.c_double)]),
    "omc_lsm_apply_mlp": (C.c_int, [_P, _P, _I64, _I64, _I, _D, _D, _D, _I, _I, _I, _P, _P, _P, _D, _D, _D, _U64,
                                    C.POINTER(Result), _P, _P]),
    "omc_lsm_apply_mlp_shard": (C.c_int, [_P, _P, _I64, _I64, _I, _D, _D, _D, _I, _I, _I, _P, _P, _P, _D, _D, _D, _U64,
                                          C.POINTER(Result), _P, _P, _I64, _I64]),
    "omc_localvol_param_count": (C.c_int, [_I, _I]),
    "omc_localvol_paths_f32": (C.c_int, [_P, _P, _I64, _I64, _I, _D, _D, _D, _D, _I, _I, _P, _D, _D, _D, _P]),
    "omc_nn_build_rows": (C.c_int, [_P, _P, _I64, _I64, _I, _D, _D, _D, _I, _P, _I64, C.POINTER(C.c_int64), _P]),
    "omc_nn_feature_stats": (C.c_int, [_P, _P, _P, _P, _I64, _D, _D, _P]),
}

# The entry points of include/omc_jump_bounds.h, an extension header of include/omc.h: SIGNATURES is
# the set that omc.h declares, and stays that set.
JUMP_BOUNDS_SIGNATURES = {
    "omc_jump_paths_f32": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Jump), _D, _P, _P, _I64]),
    "omc_price_american_bounds_jump": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Jump), _D, C.POINTER(BoundsConfig), _P,
                                                 _P, _P, _P, C.POINTER(Bounds)]),
}

# The entry points of include/omc_dividend_bounds.h, an extension header of its own.
DIVIDEND_BOUNDS_SIGNATURES = {
    "omc_dividend_paths_f32": (C.c_int, [_P, C.POINTER(Params), _D, _P, _I, _I, _P, _P, _I64]),
    "omc_price_american_bounds_div": (C.c_int, [_P, C.POINTER(Params), _D, _P, _I, C.POINTER(BoundsConfig), _P, _P, _P, _P,
                                                C.POINTER(Bounds)]),
}

# The entry points of include/omc_barrier_bounds.h, an extension header of its own.
BARRIER_BOUNDS_SIGNATURES = {
    "omc_barrier_paths_state_f32": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Barrier), _I, _P, _P, _P, _P, _I64]),
    "omc_price_american_bounds_barrier": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Barrier), C.POINTER(BoundsConfig), _P, _P,
                                                    _P, _P, C.POINTER(Bounds)]),
}

# The entry point of include/omc_dividend_greeks.h, an extension header of its own.
DIVIDEND_GREEKS_SIGNATURES = {
    "omc_price_american_div_greeks": (C.c_int, [_P, C.POINTER(Params), _D, _P, _I, _D, _P, _P, C.POINTER(DivGreeks)]),
}

# The entry point of include/omc_chain_bounds.h, an extension header of its own.
CHAIN_BOUNDS_SIGNATURES = {
    "omc_price_american_chain_bounds": (C.c_int, [_P, C.POINTER(Params), C.POINTER(ChainEntry), _I, C.POINTER(BoundsConfig),
                                                  _P, _P, _P, _P, C.POINTER(Bounds), C.POINTER(ChainBoundsInfo)]),
}

# The entry point of include/omc_jump_greeks.h, an extension header of its own.
JUMP_GREEKS_SIGNATURES = {
    "omc_price_american_jump_greeks": (C.c_int, [_P, C.POINTER(Params), C.POINTER(Jump), _D, _D, _P, _P,
                                                 C.POINTER(JumpGreeks)]),
}

# The entry point of include/omc_chain_greeks.h, an extension header of its own.
CHAIN_GREEKS_SIGNATURES = {
    "omc_price_american_chain_greeks": (C.c_int, [_P, C.POINTER(Params), C.POINTER(ChainEntry), _I, _D, _P, _P,
                                                  C.POINTER(Greeks), C.POINTER(ChainGreeksInfo)]),
}

_lib = None
_lib_lock = threading.Lock()
_hip_runtime = None


def _preload_hip_runtime():
    """One process must use ONE HIP runtime.  The PyTorch-ROCm wheel bundles its own
    libamdhip64.so.7 / libhsa-runtime64 (torch/lib); if libomc.so pulled in /opt/rocm's copy
    first, a later `import torch` would find the GPU already owned by a different runtime and
    report no devices.  So when that wheel is installed, its runtime is dlopen'ed (RTLD_GLOBAL,
    without importing torch) before libomc.so, whose NEEDED libamdhip64.so.7 then resolves to
    the already-loaded copy.  OMC_HIP_RUNTIME=system forces /opt/rocm; =<path> forces a file."""
    global _hip_runtime
    if _hip_runtime is not None:
        return
    import importlib.util
    import sys
    mode = os.environ.get("OMC_HIP_RUNTIME", "auto")
    if mode == "system" or "torch" in sys.modules:
        return
    cand = None
    if mode not in ("auto", "torch") and os.path.exists(mode):
        cand = mode
    else:
        try:
            spec = importlib.util.find_spec("torch")
        except (ImportError, ValueError):
            spec = None
        if spec is not None and spec.submodule_search_locations:
            p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
            if os.path.exists(p):
                cand = p
    if cand:
        try:
            _hip_runtime = C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            _hip_runtime = None


def load_library(build_if_missing: bool = True):
    """dlopen libomc.so (building it in-tree first if needed).  No HIP call happens here."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        path = _build.LIB
        if not os.path.exists(path) or (build_if_missing and _build._stale()):
            if not build_if_missing:
                raise OmcError(f"{path} is missing: run `python -m options_model_amd._build`")
            try:
                path = _build.build()
            except Exception as e:  # stale-but-present library is still usable on a box w/o hipcc
                if not os.path.exists(_build.LIB):
                    raise OmcError(f"libomc.so is missing and cannot be built: {e}") from e
                path = _build.LIB
        _preload_hip_runtime()
        lib = C.CDLL(path)
        for name, (res, args) in {**SIGNATURES, **JUMP_BOUNDS_SIGNATURES, **DIVIDEND_BOUNDS_SIGNATURES,
                                  **BARRIER_BOUNDS_SIGNATURES, **DIVIDEND_GREEKS_SIGNATURES, **CHAIN_BOUNDS_SIGNATURES,
                                  **JUMP_GREEKS_SIGNATURES, **CHAIN_GREEKS_SIGNATURES}.items():
            fn = getattr(lib, name)  # AttributeError = symbol missing = broken build
            fn.restype = res
            fn.argtypes = args
        if lib.omc_abi_version() != ABI_VERSION:
            raise OmcError("libomc.so ABI version mismatch: rebuild the library")
        _lib = lib
        return lib


def _check(lib, rc):
    if rc == 0:
        return
    msg = (lib.omc_last_error() or b"").decode(errors="replace")
    if rc in DIVIDEND_ERRORS:
        raise DividendError(rc, msg)
    if rc < 0:
        raise ValueError(msg)
    raise OmcError(f"HIP error {rc}: {msg}")


def comm_unique_id() -> bytes:
    """Rank 0: a fresh RCCL unique id (128 bytes) for Context.comm_init on every rank."""
    lib = load_library()
    buf = C.create_string_buffer(128)
    _check(lib, lib.omc_comm_unique_id(buf, 128))
    return buf.raw


def dividend_array(dividends):
    """[(t, amount) | (t, amount, kind)] -> a ctypes array of omc_dividend (or None when empty) and its length; a bare
    (t, amount) is a cash dividend; kind: a key of DIVIDEND_KINDS or its code."""
    items = []
    for d in dividends:
        if len(d) not in (2, 3):
            raise ValueError("a dividend is (t, amount) or (t, amount, kind).")
        t, amount, kind = (tuple(d) + ("cash",))[:3]
        e = Dividend()
        e.t, e.amount = float(t), float(amount)
        e.kind = DIVIDEND_KINDS.get(kind, -1) if isinstance(kind, str) else int(kind)
        items.append(e)
    return ((Dividend * len(items))(*items) if items else None), len(items)


def dividend_schedule(params: Params, q, dividends):
    """omc_dividend_schedule -> (mul float32 [n_steps+1], cash float32 [n_steps+1], has bool [n_steps+1]): the per-step
    table of a dividend schedule and the argument checks of Context.price_american_div.  Host only: no GPU is needed."""
    lib = load_library()
    arr, n = dividend_array(dividends)
    N = max(int(params.n_steps), 0)
    mul, cash, has = np.empty(N + 1, np.float32), np.empty(N + 1, np.float32), np.empty(N + 1, np.int32)
    _check(lib, lib.omc_dividend_schedule(C.byref(params), float(q), arr, n, mul.ctypes.data, cash.ctypes.data,
                                          has.ctypes.data))
    return mul, cash, has.astype(bool)


def make_jump(jump) -> Jump:
    """(lambda, mu_j, sigma_j) or a Jump -> Jump"""
    if isinstance(jump, Jump):
        return jump
    lam, mu, sig = jump
    return Jump(float(lam), float(mu), float(sig))


def make_barrier(kind, H, monitoring="discrete", american=True) -> Barrier:
    """omc_barrier of `kind` (a key of BARRIER_KINDS or its code; an unknown key becomes -1, which the library refuses)"""
    b = Barrier()
    b.kind = BARRIER_KINDS.get(kind, -1) if isinstance(kind, str) else int(kind)
    b.monitoring = MONITORING.get(monitoring, -1) if isinstance(monitoring, str) else int(monitoring)
    b.american = int(bool(american))
    b.H = float(H)
    return b


def jump_table(params: Params, jump, q=0.0):
    """omc_jump_table -> (thr uint32 [16], kappa, drift_rate): the Poisson thresholds of a step, the compensator and
    the generator's drift rate, after the argument checks of Context.price_american_jump.  jump: (lambda, mu_j,
    sigma_j).  Host only: no GPU is needed."""
    lib = load_library()
    thr = np.empty(16, np.uint32)
    kappa, rate = C.c_double(), C.c_double()
    _check(lib, lib.omc_jump_table(C.byref(params), C.byref(make_jump(jump)), float(q), thr.ctypes.data, C.byref(kappa),
                                   C.byref(rate)))
    return thr, kappa.value, rate.value


def make_basket(spots, sigmas, yields=None, weights=None, correlation=None, kind="basket") -> Basket:
    """per-asset sequences, a [d][d] correlation (None: identity) and a kind (a key of BASKET_KINDS or its code) -> Basket.
    Defaults: yields 0, weights 1.  Only the shapes are checked here; the values are the library's to refuse."""
    S0 = np.atleast_1d(np.asarray(spots, np.float64))
    d = S0.size
    if S0.ndim != 1 or not 1 <= d <= BASKET_MAX_ASSETS:
        raise ValueError(f"a basket has 1 .. {BASKET_MAX_ASSETS} assets.")

    def per_asset(x, default, name):
        a = np.full(d, default, np.float64) if x is None else np.atleast_1d(np.asarray(x, np.float64))
        if a.shape != (d,):
            raise ValueError(f"{name} must have one entry per asset ({d}).")
        return a
    rho = np.eye(d) if correlation is None else np.asarray(correlation, np.float64)
    if rho.shape != (d, d):
        raise ValueError(f"correlation must be a {d} x {d} matrix.")
    b = Basket()
    b.n_assets = d
    b.kind = BASKET_KINDS.get(kind, -1) if isinstance(kind, str) else int(kind)
    b.S0[:d], b.sigma[:d] = list(S0), list(per_asset(sigmas, 0.0, "sigmas"))
    b.q[:d], b.w[:d] = list(per_asset(yields, 0.0, "yields")), list(per_asset(weights, 1.0, "weights"))
    b.rho[:d * d] = list(rho.ravel())
    return b


def basket_table(params: Params, basket: Basket):
    """omc_basket_table -> (L float64 [d][d] lower Cholesky factor, a float32 [d], b float32 [d], x0, (G0, sigma_G, q_G)),
    after the argument checks of Context.price_american_basket.  Host only: no GPU is needed."""
    lib = load_library()
    d = min(max(int(basket.n_assets), 1), BASKET_MAX_ASSETS)
    Lp, a, b = np.zeros(d * (d + 1) // 2), np.zeros(d, np.float32), np.zeros(d, np.float32)
    x0, geo = C.c_double(), np.zeros(3)
    _check(lib, lib.omc_basket_table(C.byref(params), C.byref(basket), Lp.ctypes.data, a.ctypes.data, b.ctypes.data,
                                     C.byref(x0), geo.ctypes.data))
    L = np.zeros((d, d))
    L[np.tril_indices(d)] = Lp
    return L, a, b, x0.value, tuple(geo)


def device_count() -> int:
    lib = load_library()
    n = C.c_int(0)
    rc = lib.omc_device_count(C.byref(n))
    return n.value if rc == 0 else 0


class DeviceArray:
    """A device allocation owned by a Context (freed with it or explicitly)."""

    def __init__(self, ctx, shape, dtype):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        _check(ctx.lib, ctx.lib.omc_alloc(ctx.handle, self.nbytes, C.byref(p)))
        self.ptr = p.value
        ctx._arrays.add(self)

    def to_host(self):
        out = np.empty(self.shape, self.dtype)
        _check(self.ctx.lib, self.ctx.lib.omc_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr,
                                                          self.nbytes))
        return out

    def from_host(self, a):
        a = np.ascontiguousarray(a, self.dtype)
        assert a.shape == self.shape, (a.shape, self.shape)
        _check(self.ctx.lib, self.ctx.lib.omc_memcpy_h2d(self.ctx.handle, self.ptr, a.ctypes.data,
                                                          self.nbytes))
        return self

    def free(self):
        if self.ptr:
            self.ctx.lib.omc_free(self.ctx.handle, self.ptr)
            self.ptr = None
            self.ctx._arrays.discard(self)


class Context:
    """One per (process, device).  Calls on a context are serialised by the caller."""

    _bounds_every = 0  # option "bounds_exercise_every" as last set through this object (the ABI has no getter)
    _bounds_cv = 0     # option "bounds_control_variate", likewise
    _bounds_check = 0  # option "bounds_suboptimality", likewise
    _MIRRORED = {"bounds_exercise_every": "_bounds_every", "bounds_control_variate": "_bounds_cv",
                 "bounds_suboptimality": "_bounds_check"}

    def __init__(self, device: int = 0, stream: int | None = None):
        self.lib = load_library()
        h = C.c_void_p()
        _check(self.lib, self.lib.omc_ctx_create(int(device), C.c_void_p(stream) if stream else None,
                                                  C.byref(h)))
        self.handle = h
        self.device = device
        self._arrays = set()
        self._hook = None

    # -- housekeeping
    def close(self):
        if self.handle:
            for a in list(self._arrays):
                a.free()
            self.lib.omc_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def empty(self, shape, dtype=np.float32):
        return DeviceArray(self, shape, dtype)

    def to_device(self, a, dtype=None):
        a = np.ascontiguousarray(a, dtype or a.dtype)
        return DeviceArray(self, a.shape, a.dtype).from_host(a)

    def sync(self):
        _check(self.lib, self.lib.omc_sync(self.handle))

    def set_option(self, key: str, value: int):
        _check(self.lib, self.lib.omc_set_option(self.handle, key.encode(), int(value)))
        if key in self._MIRRORED:
            setattr(self, self._MIRRORED[key], int(value))

    def set_allreduce_hook(self, fn):
        """fn(dptr:int, count:int) -> None must sum-all-reduce `count` device doubles in place."""
        if fn is None:
            self._hook = None
            _check(self.lib, self.lib.omc_set_allreduce_hook(self.handle, C.cast(None, ALLREDUCE_FN), None))
            return

        def tramp(_user, dptr, count):
            try:
                fn(dptr, count)
                return 0
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1

        self._hook = ALLREDUCE_FN(tramp)
        _check(self.lib, self.lib.omc_set_allreduce_hook(self.handle, self._hook, None))

    # -- RNG taps
    def philox4x32_10(self, ctr_key):
        a = np.ascontiguousarray(ctr_key, np.uint32).reshape(-1, 6)
        out = np.empty((a.shape[0], 4), np.uint32)
        _check(self.lib, self.lib.omc_philox4x32_10(self.handle, a.ctypes.data, out.ctypes.data,
                                                     a.shape[0]))
        return out

    def gbm_normals(self, n_pairs, n_steps, seed, stream=0, pair_offset=0):
        Z = self.empty((n_steps, n_pairs), np.float32)
        _check(self.lib, self.lib.omc_gbm_normals_f32(self.handle, Z.ptr, n_pairs, n_pairs, n_steps,
                                                       seed, stream, pair_offset))
        return Z

    # -- paths (device matrices [n_steps+1][n_paths], ld == n_paths)
    def gbm_paths(self, n_paths, n_steps, S0, r, sigma, T, seed, stream=0, pair_offset=0,
                  antithetic=True, out=None):
        S = out if out is not None else self.empty((n_steps + 1, n_paths), np.float32)
        _check(self.lib, self.lib.omc_gbm_paths_f32(self.handle, S.ptr, S.shape[1], n_paths, n_steps,
                                                     S0, r, sigma, T, seed, stream, pair_offset,
                                                     int(antithetic)))
        return S

    def heston_paths(self, n_paths, n_steps, S0, r, T, v0, kappa, theta, xi, rho, seed, stream=0,
                     pair_offset=0, scheme=0, out=None):
        S = out if out is not None else self.empty((n_steps + 1, n_paths), np.float32)
        _check(self.lib, self.lib.omc_heston_paths_f32(self.handle, S.ptr, S.shape[1], n_paths,
                                                        n_steps, S0, r, T, v0, kappa, theta, xi, rho,
                                                        seed, stream, pair_offset, scheme))
        return S

    def heston_paths_sv(self, n_paths, n_steps, S0, r, T, v0, kappa, theta, xi, rho, seed, stream=0,
                        pair_offset=0, scheme=0):
        """heston_paths with the variance state kept (omc_heston_paths_sv_f32) -> (S, V), both [n_steps+1][n_paths]."""
        S = self.empty((n_steps + 1, n_paths), np.float32)
        V = self.empty((n_steps + 1, n_paths), np.float32)
        _check(self.lib, self.lib.omc_heston_paths_sv_f32(self.handle, S.ptr, V.ptr, S.shape[1], n_paths,
                                                           n_steps, S0, r, T, v0, kappa, theta, xi, rho,
                                                           seed, stream, pair_offset, scheme))
        return S, V

    def jump_paths(self, params: Params, jump, q=0.0, want_v=False):
        """The jump generator's matrix (omc_jump_paths_f32) of params.n_paths antithetic paths at (params.seed,
        params.stream, params.pair_offset), started at (params.S0, params.v0) -> device S [n_steps+1][n_paths], or
        (S, V) with want_v (Heston: the variance state after every step).  jump: (lambda, mu_j, sigma_j); q: dividend
        yield.  params.v0 of Heston schemes 0 .. 2 is a start state: a stored full-truncation state may be negative."""
        n_paths, n_steps = int(params.n_paths), int(params.n_steps)
        S = self.empty((n_steps + 1, n_paths), np.float32)
        V = self.empty((n_steps + 1, n_paths), np.float32) if want_v else None
        try:
            _check(self.lib, self.lib.omc_jump_paths_f32(self.handle, C.byref(params), C.byref(make_jump(jump)), float(q),
                                                          S.ptr, V.ptr if want_v else None, S.shape[1]))
        except Exception:
            S.free()
            if want_v:
                V.free()
            raise
        return (S, V) if want_v else S

    def dividend_paths(self, params: Params, q=0.0, dividends=(), step_offset=0, want_v=False):
        """The dividend generator's matrix (omc_dividend_paths_f32) of params.n_paths antithetic paths at (params.seed,
        params.stream, params.pair_offset), started at (params.S0, params.v0) at date step_offset -> device S
        [n_steps+1][n_paths], or (S, V) with want_v (Heston: the variance state after every step).  q: dividend yield;
        dividends: as price_american_div takes them; row k takes the schedule's entry of step step_offset + k.  params.v0 of
        Heston schemes 0 .. 2 is a start state: a stored full-truncation state may be negative."""
        arr, n = dividend_array(dividends)
        n_paths, n_steps = int(params.n_paths), int(params.n_steps)
        S = self.empty((n_steps + 1, n_paths), np.float32)
        V = self.empty((n_steps + 1, n_paths), np.float32) if want_v else None
        try:
            _check(self.lib, self.lib.omc_dividend_paths_f32(self.handle, C.byref(params), float(q), arr, n,
                                                              int(step_offset), S.ptr, V.ptr if want_v else None,
                                                              S.shape[1]))
        except Exception:
            S.free()
            if want_v:
                V.free()
            raise
        return (S, V) if want_v else S

    def barrier_paths_state(self, params: Params, kind, H, start_hit=False, monitoring="discrete"):
        """The barrier generator with its paths' state kept (omc_barrier_paths_state_f32) of params.n_paths antithetic paths
        at (params.seed, params.stream, params.pair_offset), started at (params.S0, params.v0) -> device (E, S, V, hit): the
        encoded index and the real spots [n_steps+1][n_paths], under Heston the variance state (GBM: None), and the int32
        first-hit step of every path (0 = never).  kind: a key of BARRIER_KINDS or its code.  start_hit: a restart from a
        state that has been hit (row 0 is encoded as hit, every entry of hit is -1, S0 may lie beyond the barrier);
        params.v0 of a Heston call is a start state: a stored full-truncation state may be negative."""
        n_paths, n_steps = int(params.n_paths), int(params.n_steps)
        heston = int(params.model) == MODELS["heston"]
        arrs = [self.empty((n_steps + 1, n_paths), np.float32), self.empty((n_steps + 1, n_paths), np.float32),
                self.empty((n_steps + 1, n_paths), np.float32) if heston else None, self.empty((n_paths,), np.int32)]
        E, S, V, hit = arrs
        try:
            _check(self.lib, self.lib.omc_barrier_paths_state_f32(self.handle, C.byref(params),
                                                                   C.byref(make_barrier(kind, H, monitoring)),
                                                                   int(bool(start_hit)), E.ptr, S.ptr, V.ptr if heston else None,
                                                                   hit.ptr, E.shape[1]))
        except Exception:
            for a in arrs:
                if a is not None:
                    a.free()
            raise
        return E, S, V, hit

    def gbm_paths_from_normals(self, z_half, S0, r, sigma, T, antithetic=True):
        z = self.to_device(z_half, np.float32)
        N, P = z.shape
        M = 2 * P if antithetic else P
        S = self.empty((N + 1, M), np.float32)
        _check(self.lib, self.lib.omc_gbm_paths_from_normals_f32(self.handle, S.ptr, M, M, N, S0, r,
                                                                  sigma, T, z.ptr, P, int(antithetic)))
        z.free()
        return S

    def heston_paths_from_normals(self, z1_half, z2_half, S0, r, T, v0, kappa, theta, xi, rho,
                                  scheme=0):
        z1 = self.to_device(z1_half, np.float32)
        z2 = self.to_device(z2_half, np.float32)
        N, P = z1.shape
        S = self.empty((N + 1, 2 * P), np.float32)
        try:
            rc = self.lib.omc_heston_paths_from_normals_f32(
                self.handle, S.ptr, 2 * P, 2 * P, N, S0, r, T, v0, kappa, theta, xi, rho, z1.ptr, z2.ptr,
                P, scheme)
        finally:
            z1.free()
            z2.free()
        if rc != 0:
            S.free()
        _check(self.lib, rc)  # ValueError for a refusal (-5: rho outside [-1, 1]; scheme 3 with v0 < 0)
        return S

    # -- backward induction on a device path matrix
    def lsm_poly(self, S, K, r, T, is_put, semantics="reference", want_state=False, n_paths=None):
        N = S.shape[0] - 1
        ld = S.shape[1]
        M = ld if n_paths is None else n_paths
        res = Result()
        betas = np.zeros((N + 1, 4))
        sx = np.zeros(M, np.float32) if want_state else None
        tex = np.zeros(M, np.int32) if want_state else None
        ptr = S.ptr if isinstance(S, DeviceArray) else int(S.data_ptr())
        _check(self.lib, self.lib.omc_lsm_poly(self.handle, ptr, ld, M, N, K, r, T, int(is_put),
                                                SEMANTICS[semantics], C.byref(res), betas.ctypes.data,
                                                sx.ctypes.data if want_state else None,
                                                tex.ctypes.data if want_state else None))
        d = res.as_dict()
        d.update(betas=betas[:, :3], nitm=betas[:, 3].astype(np.int64), sx=sx, tex=tex)
        return d

    def lsm_ols7(self, S, K, r, T, is_put, want_state=False, n_paths=None):
        """Two-pass flow with the global least-squares fit on the reference's 7 features (omc_lsm_ols7) on a device path
        matrix -> result dict + weights [7], feat_mean / feat_std [7], y_mean, y_std (+ sx, tex if want_state)."""
        N = S.shape[0] - 1
        ld = S.shape[1]
        M = ld if n_paths is None else n_paths
        res = Result()
        w = np.zeros(7)
        st = np.zeros(16)
        sx = np.zeros(M, np.float32) if want_state else None
        tex = np.zeros(M, np.int32) if want_state else None
        ptr = S.ptr if isinstance(S, DeviceArray) else int(S.data_ptr())
        _check(self.lib, self.lib.omc_lsm_ols7(self.handle, ptr, ld, M, N, K, r, T, int(is_put), C.byref(res), w.ctypes.data,
                                                st.ctypes.data, sx.ctypes.data if want_state else None,
                                                tex.ctypes.data if want_state else None))
        d = res.as_dict()
        d.update(weights=w, feat_mean=st[:7].copy(), feat_std=st[7:14].copy(), y_mean=float(st[14]), y_std=float(st[15]),
                 sx=sx, tex=tex)
        return d

    def lsm_apply_frozen(self, S, K, r, T, is_put, betas4, want_state=True):
        N, M = S.shape[0] - 1, S.shape[1]
        b = np.ascontiguousarray(betas4, np.float64)
        assert b.shape == (N + 1, 4)
        res = Result()
        sx = np.zeros(M, np.float32) if want_state else None
        tex = np.zeros(M, np.int32) if want_state else None
        _check(self.lib, self.lib.omc_lsm_apply_frozen(self.handle, S.ptr, M, M, N, K, r, T,
                                                        int(is_put), b.ctypes.data, C.byref(res),
                                                        sx.ctypes.data if want_state else None,
                                                        tex.ctypes.data if want_state else None))
        d = res.as_dict()
        d.update(sx=sx, tex=tex)
        return d

    def lsm_apply_values(self, S, K, r, T, is_put, cont, semantics="reference", want_state=True):
        """Per-step sweep driven by a device float32 matrix of continuation values [N+1][M]."""
        N, M = S.shape[0] - 1, S.shape[1]
        assert cont.shape == (N + 1, M) and cont.dtype == np.float32
        res = Result()
        sx = np.zeros(M, np.float32) if want_state else None
        tex = np.zeros(M, np.int32) if want_state else None
        _check(self.lib, self.lib.omc_lsm_apply_values(self.handle, S.ptr, M, M, N, K, r, T, int(is_put),
                                                        SEMANTICS[semantics], cont.ptr, M, C.byref(res),
                                                        sx.ctypes.data if want_state else None,
                                                        tex.ctypes.data if want_state else None))
        d = res.as_dict()
        d.update(sx=sx, tex=tex)
        return d

    def lsm_contnet(self, S, K, r, T, is_put, nn_hidden=32, nn_epochs=10, nn_lr=1e-3, nn_seed=0, want_state=True):
        """The reference's v1 / v2 per-step flow (fresh ContNet per step) on a device path matrix."""
        N, M = S.shape[0] - 1, S.shape[1]
        res = Result()
        sx = np.zeros(M, np.float32) if want_state else None
        tex = np.zeros(M, np.int32) if want_state else None
        _check(self.lib, self.lib.omc_lsm_contnet(self.handle, S.ptr, M, M, N, K, r, T, int(is_put), int(nn_hidden),
                                                   int(nn_epochs), float(nn_lr), int(nn_seed) & (2**64 - 1),
                                                   C.byref(res), sx.ctypes.data if want_state else None,
                                                   tex.ctypes.data if want_state else None))
        d = res.as_dict()
        d.update(sx=sx, tex=tex)
        return d

    def contnet_init_params(self, nn_hidden, t, nn_seed=0):
        """Initial parameters of step t's net as a dict of torch-shaped arrays (w0 [h,1], b0, w1 [h,h], b1, w2 [1,h], b2)."""
        H = 32 if nn_hidden <= 32 else 64 if nn_hidden <= 64 else 128
        n = 8 * H + H * H + 2 * H + 1
        flat = np.zeros(n, np.float32)
        _check(self.lib, self.lib.omc_contnet_init_params(self.handle, int(nn_hidden), int(t),
                                                           int(nn_seed) & (2**64 - 1), flat.ctypes.data, n))
        h = int(nn_hidden)
        l0 = flat[:8 * H].reshape(H, 8)
        w1 = flat[8 * H:8 * H + H * H].reshape(H, H)
        b1 = flat[8 * H + H * H:8 * H + H * H + H]
        wo = flat[8 * H + H * H + H:8 * H + H * H + 2 * H]
        return dict(w0=l0[:h, :1].copy(), b0=l0[:h, 7].copy(), w1=w1[:h, :h].copy(), b1=b1[:h].copy(),
                    w2=wo[:h].reshape(1, h).copy(), b2=flat[-1:].copy(), flat=flat)

    def price_american_contnet(self, params: Params, nn_hidden=32, nn_epochs=10, nn_lr=1e-3, nn_seed=0):
        res = Result()
        _check(self.lib, self.lib.omc_price_american_contnet(self.handle, C.byref(params), int(nn_hidden),
                                                              int(nn_epochs), float(nn_lr),
                                                              int(nn_seed) & (2**64 - 1), C.byref(res)))
        return res.as_dict()

    # -- native RCCL communicator (no torch): see include/omc.h
    def comm_init(self, rank: int, world: int, uid: bytes):
        buf = C.create_string_buffer(bytes(uid), 128)
        _check(self.lib, self.lib.omc_comm_init(self.handle, int(rank), int(world), buf, 128))

    def comm_destroy(self):
        _check(self.lib, self.lib.omc_comm_destroy(self.handle))

    def comm_info(self):
        """-> (rank, world) of the live communicator; world == 0: none."""
        r, w = C.c_int(0), C.c_int(0)
        _check(self.lib, self.lib.omc_comm_info(self.handle, C.byref(r), C.byref(w)))
        return r.value, w.value

    def device_info(self) -> dict:
        """-> dict(device=HIP ordinal, pci_bus_id="0000:c1:00.0", name=...) of the card this context runs on."""
        dev = C.c_int(-1)
        pci, name = C.create_string_buffer(64), C.create_string_buffer(256)
        _check(self.lib, self.lib.omc_ctx_device_info(self.handle, C.byref(dev), pci, 64, name, 256))
        return dict(device=dev.value, pci_bus_id=pci.value.decode(), name=name.value.decode())

    def comm_allreduce(self, values, op="sum"):
        a = np.ascontiguousarray(values, np.float64).copy()
        _check(self.lib, self.lib.omc_comm_allreduce_f64(self.handle, a.ctypes.data, a.size, 1 if op == "max" else 0))
        return a

    # -- direct peer exchange of the per-step moments (include/omc.h)
    def p2p_export(self) -> bytes:
        buf = C.create_string_buffer(64)
        _check(self.lib, self.lib.omc_p2p_export(self.handle, buf, 64))
        return buf.raw

    def p2p_connect(self, rank: int, world: int, handles: bytes):
        buf = C.create_string_buffer(bytes(handles), 64 * int(world))
        _check(self.lib, self.lib.omc_p2p_connect(self.handle, int(rank), int(world), buf, 64 * int(world)))

    def p2p_disconnect(self):
        _check(self.lib, self.lib.omc_p2p_disconnect(self.handle))

    def p2p_status(self):
        """-> (connected, world, sticky error word)"""
        a, b, e = C.c_int(0), C.c_int(0), C.c_uint64(0)
        _check(self.lib, self.lib.omc_p2p_status(self.handle, C.byref(a), C.byref(b), C.byref(e)))
        return bool(a.value), b.value, e.value

    # -- fused pricing
    def price_american(self, params: Params, keep_paths: DeviceArray | None = None):
        res = Result()
        _check(self.lib, self.lib.omc_price_american(
            self.handle, C.byref(params), C.byref(res), keep_paths.ptr if keep_paths else None,
            keep_paths.shape[1] if keep_paths else 0))
        return res.as_dict()

    def pass2_tables_check(self, is_put, K, betas, cK, irregular_every=0):
        """omc_pass2_tables_check -> (mismatches [N+1][2] int64, irregular [N+1] bool): pass 2's exercise tables of the fits
        `betas` [N+1][4] and cK [N+1] against the float64 decisions at every non-negative float32 spot."""
        b = np.ascontiguousarray(betas, np.float64)
        ck = np.ascontiguousarray(cK, np.float64)
        N = b.shape[0] - 1
        if b.shape != (N + 1, 4) or ck.shape != (N + 1,):
            raise ValueError("betas must be [N+1][4] and cK [N+1].")
        mism = np.zeros((N + 1, 2), np.int64)
        irr = np.zeros(N + 1, np.int32)
        _check(self.lib, self.lib.omc_pass2_tables_check(self.handle, int(bool(is_put)), float(K), N, b.ctypes.data,
                                                         ck.ctypes.data, int(irregular_every), mism.ctypes.data,
                                                         irr.ctypes.data))
        return mism, irr.astype(bool)

    def price_american_greeks(self, params: Params, bump=0.01, betas=None, want_betas=False):
        """Frozen-policy pathwise Greeks of the two-pass flow (omc_price_american_greeks) -> dict: the base pricing's keys
        (as price_american returns them) plus delta, gamma, vega, rho, theta (raw units), se_*, bump, price_up, price_down,
        n_exercised_up / _down, ms_greeks; `betas` [n_steps+1][4] freezes a given policy; want_betas adds the policy used."""
        N = int(params.n_steps)
        b = None
        if betas is not None:
            b = np.ascontiguousarray(betas, np.float64)
            if b.shape != (N + 1, 4):
                raise ValueError(f"betas must have shape ({N + 1}, 4), got {b.shape}.")
        bo = np.zeros((N + 1, 4)) if want_betas else None
        g = Greeks()
        _check(self.lib, self.lib.omc_price_american_greeks(self.handle, C.byref(params), float(bump),
                                                             b.ctypes.data if b is not None else None,
                                                             bo.ctypes.data if bo is not None else None, C.byref(g)))
        d = _with_base(g)
        if want_betas:
            d["betas"] = bo
        return d

    def price_barrier(self, params: Params, kind, H, monitoring="discrete", american=True,
                      keep_paths: DeviceArray | None = None):
        """Barrier option (omc_price_barrier) -> dict: the base pricing's keys (American: as price_american returns them on
        the encoded matrix; European: the option of `kind`) plus euro_out, euro_out_se, euro_in, euro_in_se, hit_prob,
        ms_barrier_paths.  kind: a key of BARRIER_KINDS or its code; monitoring: "discrete" / "continuous" (GBM);
        keep_paths: device [n_steps+1][ld] receiving the encoded matrix."""
        b = Barrier()
        b.kind = BARRIER_KINDS.get(kind, -1) if isinstance(kind, str) else int(kind)
        b.monitoring = MONITORING.get(monitoring, -1) if isinstance(monitoring, str) else int(monitoring)
        b.american = int(bool(american))
        b.H = float(H)
        out = BarrierResult()
        _check(self.lib, self.lib.omc_price_barrier(self.handle, C.byref(params), C.byref(b), C.byref(out),
                                                     keep_paths.ptr if keep_paths else None,
                                                     keep_paths.shape[1] if keep_paths else 0))
        return _with_base(out)

    def price_american_div(self, params: Params, q=0.0, dividends=(), S_keep: DeviceArray | None = None):
        """American option on a stock with a dividend yield q and discrete dividends (omc_price_american_div) -> dict: the
        base pricing's keys (as price_american returns them) plus ms_div_paths, n_div_steps, first_div_step.  dividends:
        [(t, amount) | (t, amount, "cash" | "proportional")]; S_keep: device [n_steps+1][ld] receiving the path matrix."""
        arr, n = dividend_array(dividends)
        out = DivResult()
        _check(self.lib, self.lib.omc_price_american_div(self.handle, C.byref(params), float(q), arr, n, C.byref(out),
                                                          S_keep.ptr if S_keep else None,
                                                          S_keep.shape[1] if S_keep else 0))
        return _with_base(out)

    def price_american_dividend_greeks(self, params: Params, q=0.0, dividends=(), bump=0.01, betas=None, want_betas=False):
        """Frozen-policy pathwise Greeks of price_american_div's product (omc_price_american_div_greeks) -> dict: the base
        pricing's keys plus delta, gamma, vega, rho, theta, epsilon (dV/dq; raw units), se_*, bump, price_up, price_down,
        n_exercised_up / _down, ms_greeks, n_div_steps, first_div_step.  One forward sweep on regenerated paths replaces
        pass 2.  Heston gives delta and gamma, the others are NaN.  `betas` [n_steps+1][4] freezes a given policy (an
        all-n <= 0 table: the European option); want_betas adds the policy used."""
        arr, n = dividend_array(dividends)
        N = int(params.n_steps)
        b = None
        if betas is not None:
            b = np.ascontiguousarray(betas, np.float64)
            if b.shape != (N + 1, 4):
                raise ValueError(f"betas must have shape ({N + 1}, 4), got {b.shape}.")
        bo = np.zeros((N + 1, 4)) if want_betas else None
        out = DivGreeks()
        _check(self.lib, self.lib.omc_price_american_div_greeks(self.handle, C.byref(params), float(q), arr, n, float(bump),
                                                                 b.ctypes.data if b is not None else None,
                                                                 bo.ctypes.data if bo is not None else None, C.byref(out)))
        d = _with_base(out.g)
        d.update(epsilon=out.epsilon, se_epsilon=out.se_epsilon, n_div_steps=out.n_div_steps,
                 first_div_step=out.first_div_step)
        if want_betas:
            d["betas"] = bo
        return d

    def price_american_jump(self, params: Params, jump, q=0.0, S_keep: DeviceArray | None = None):
        """American option under jump-diffusion (omc_price_american_jump: Merton on GBM, Bates on Heston) -> dict: the
        base pricing's keys (as price_american returns them) plus ms_jump_paths, kappa, drift_rate, n_thresholds.
        jump: (lambda, mu_j, sigma_j); q: dividend yield; S_keep: device [n_steps+1][ld] receiving the path matrix."""
        out = JumpResult()
        _check(self.lib, self.lib.omc_price_american_jump(self.handle, C.byref(params), C.byref(make_jump(jump)), float(q),
                                                           C.byref(out), S_keep.ptr if S_keep else None,
                                                           S_keep.shape[1] if S_keep else 0))
        return _with_base(out)

    def price_american_jump_greeks(self, params: Params, jump, q=0.0, bump=0.01, betas=None, want_betas=False):
        """Frozen-policy Greeks of price_american_jump's product (omc_price_american_jump_greeks) -> dict: the base
        pricing's keys plus delta, gamma, vega, rho, theta, epsilon (dV/dq), dlambda, dmu_j, dsigma_j, theta_score (raw
        units), se_*, bump, price_up, price_down, n_exercised_up / _down, ms_greeks, kappa, drift_rate, n_jumps.  One
        forward sweep on regenerated paths replaces pass 2; dlambda and theta carry a score-function term.  Heston (Bates)
        gives delta and gamma, the others are NaN; at lambda = 0 dlambda is NaN.  `betas` [n_steps+1][4] freezes a given
        policy (an all-n <= 0 table: the European option); want_betas adds the policy used."""
        N = int(params.n_steps)
        b = None
        if betas is not None:
            b = np.ascontiguousarray(betas, np.float64)
            if b.shape != (N + 1, 4):
                raise ValueError(f"betas must have shape ({N + 1}, 4), got {b.shape}.")
        bo = np.zeros((N + 1, 4)) if want_betas else None
        out = JumpGreeks()
        _check(self.lib, self.lib.omc_price_american_jump_greeks(self.handle, C.byref(params), C.byref(make_jump(jump)),
                                                                  float(q), float(bump),
                                                                  b.ctypes.data if b is not None else None,
                                                                  bo.ctypes.data if bo is not None else None, C.byref(out)))
        d = _with_base(out.g)
        for name, _ in JumpGreeks._fields_[1:]:
            d[name] = getattr(out, name)
        if want_betas:
            d["betas"] = bo
        return d

    def price_american_basket(self, params: Params, basket: Basket, S_keep: DeviceArray | None = None,
                              assets_keep: DeviceArray | None = None):
        """American option on the index of several correlated GBM assets (omc_price_american_basket) -> dict: the base
        pricing's keys (as price_american returns them) plus ms_basket_paths, index0, n_assets, kind.  params.S0 and
        params.sigma are not read.  S_keep: device [n_steps+1][ld] receiving the index matrix; assets_keep: device
        [n_assets][n_steps+1][ld] receiving the asset matrices (the same ld when both are given)."""
        ld = (S_keep or assets_keep).shape[-1] if (S_keep or assets_keep) else 0
        if assets_keep is not None:
            if assets_keep.shape[:2] != (int(basket.n_assets), int(params.n_steps) + 1):
                raise ValueError("assets_keep must have shape (n_assets, n_steps + 1, ld).")
            if S_keep is not None and S_keep.shape[1] != assets_keep.shape[2]:
                raise ValueError("S_keep and assets_keep must share their leading dimension.")
        out = BasketResult()
        _check(self.lib, self.lib.omc_price_american_basket(self.handle, C.byref(params), C.byref(basket), C.byref(out),
                                                             S_keep.ptr if S_keep else None,
                                                             assets_keep.ptr if assets_keep else None, ld))
        return _with_base(out)

    def price_american_basket_greeks(self, params: Params, basket: Basket, bump=0.01, gamma=True, betas=None,
                                     want_betas=False):
        """Frozen-policy pathwise Greeks of price_american_basket (omc_price_american_basket_greeks) -> dict: the keys
        of price_american_basket (ms_pass2 = 0) plus delta, gamma, vega, se_delta, se_gamma, se_vega, price_up,
        price_down, n_exercised_up, n_exercised_down (lists, one entry per asset), rho, theta, se_rho, se_theta, bump,
        ms_greeks, gamma_on.  gamma=False: no scenario chains (gamma, se_gamma, price_up, price_down are NaN); `betas`
        [n_steps+1][4] freezes a given policy (no paths are written); want_betas adds the policy used."""
        N = int(params.n_steps)
        b = None
        if betas is not None:
            b = np.ascontiguousarray(betas, np.float64)
            if b.shape != (N + 1, 4):
                raise ValueError(f"betas must have shape ({N + 1}, 4), got {b.shape}.")
        bo = np.zeros((N + 1, 4)) if want_betas else None
        g = BasketGreeks()
        _check(self.lib, self.lib.omc_price_american_basket_greeks(self.handle, C.byref(params), C.byref(basket),
                                                                    float(bump), int(bool(gamma)),
                                                                    b.ctypes.data if b is not None else None,
                                                                    bo.ctypes.data if bo is not None else None,
                                                                    C.byref(g)))
        d = _with_base(g.base)
        n = int(g.base.n_assets)
        for k, _ in BasketGreeks._fields_:
            if k in ("base", "reserved"):
                continue
            v = getattr(g, k)
            d[k] = list(v)[:n] if hasattr(v, "__len__") else v
        if want_betas:
            d["betas"] = bo
        return d

    def price_american_bounds(self, params: Params, policy="textbook", n_lower=1_000_000, n_outer=8192, n_inner=1024,
                              stream_lower=None, stream_outer=None, stream_inner=None, betas=None, want_q=False,
                              want_samples=False, exercise_every=0, control_variate=False, suboptimality_check=None):
        """Andersen-Broadie bounds of the Bermudan game on the grid (omc_price_american_bounds) -> dict with the fields of
        omc_bounds plus `betas` (the policy used, [n_steps+1][4]) and, when asked, `q` ([n_outer][n_steps]: Q^_t) and
        `samples` ([n_outer]).  policy: a key of BOUND_POLICIES or its code; betas: the table of policy "given".  Streams
        default to params.stream + 1 / 2 / 3.
        exercise_every = k >= 2: the game with exercise at every k-th date counted back from expiry (option
        "bounds_exercise_every", set for this call and put back after it); `betas` has zero rows off the schedule and `q` is
        zero in the columns that are no scheduled date.
        control_variate=True: the Black-Scholes control variate of DESIGN.md section 26 (option "bounds_control_variate",
        set for this call and put back after it; None: the option as the context holds it): the same paths and stops,
        `lower` and `q` estimated with the discounted European value as the control.
        suboptimality_check: "off", "payoff" or "european" (a key of BOUND_CHECKS; DESIGN.md section 27, option
        "bounds_suboptimality", set for this call and put back after it; None: the option as the context holds it): inner
        simulations only where exercise is not known to be sub-optimal; `q` is zero at the skipped items, `lower` is the
        unchecked call's and `upper` is at most its value up to rounding."""
        with self._bounds_control(control_variate), self._bounds_checking(suboptimality_check):
            return self._bounds("omc_price_american_bounds", (), Bounds, params, policy, n_lower, n_outer, n_inner,
                                stream_lower, stream_outer, stream_inner, betas, want_q, want_samples,
                                exercise_every=exercise_every)

    @contextlib.contextmanager
    def _option_for_calls(self, key, value):
        """option `key` (one of _MIRRORED) = value for the calls inside, the previous value after them (None: the option
        stays as the context holds it)"""
        if value is None:
            yield
            return
        before = getattr(self, self._MIRRORED[key])
        self.set_option(key, value)
        try:
            yield
        finally:
            self.set_option(key, before)

    def _bounds_control(self, control_variate):
        """option "bounds_control_variate" = control_variate for the calls inside, the previous value after them (None: the
        option stays as the context holds it)"""
        return self._option_for_calls("bounds_control_variate", None if control_variate is None else int(bool(control_variate)))

    def _bounds_checking(self, suboptimality_check):
        """option "bounds_suboptimality" = the code of suboptimality_check for the calls inside, the previous value after
        them (None: the option stays as the context holds it)"""
        if suboptimality_check is not None and suboptimality_check not in BOUND_CHECKS:
            raise ValueError(f"suboptimality_check must be one of {list(BOUND_CHECKS)} or None.")
        return self._option_for_calls("bounds_suboptimality",
                                      None if suboptimality_check is None else BOUND_CHECKS.index(suboptimality_check))

    def _bounds_schedule(self, exercise_every):
        """option "bounds_exercise_every" = exercise_every for the calls inside, the previous value after them (None: the
        option stays as the context holds it)"""
        return self._option_for_calls("bounds_exercise_every", exercise_every)

    def price_american_bounds_heston(self, params: Params, policy="textbook", n_lower=1_000_000, n_outer=8192,
                                     n_inner=1024, stream_lower=None, stream_outer=None, stream_inner=None, betas=None,
                                     want_q=False, want_samples=False, regressors="spot", exercise_every=0,
                                     suboptimality_check=None):
        """Andersen-Broadie bounds of the Bermudan game of the discretised Heston scheme on the grid
        (omc_price_american_bounds_heston; scheme reference or full_truncation) -> the dict of price_american_bounds.  The
        policy is a function of the spot alone; the inner paths start at the outer (spot, variance) state.  Streams default
        to params.stream + 1 / 2 / 3.
        regressors="spot+variance" (cfg.regressors = 1; policy "textbook" or "given", at most 512 steps): the policy sees the
        spot and the variance state, w = V / max(v0, theta) - 1, and `betas` (given and returned) is [n_steps+1][8] =
        c0 .. c5, n, 0.  A key of HESTON_BOUND_REGRESSORS or its code.
        exercise_every: as price_american_bounds takes it, with regressors "spot" (the spot + variance policy refuses a
        schedule with -38).
        suboptimality_check: as price_american_bounds takes it, "off" or "payoff" with regressors "spot" (anything else is
        refused with -40)."""
        if isinstance(regressors, str):
            regressors = heston_regressors_code(regressors)
        with self._bounds_checking(suboptimality_check):
            return self._bounds("omc_price_american_bounds_heston", (), Bounds, params, policy, n_lower, n_outer, n_inner,
                                stream_lower, stream_outer, stream_inner, betas, want_q, want_samples,
                                8 if int(regressors) == 1 else 4, regressors=int(regressors), exercise_every=exercise_every)

    def price_american_bounds_jump(self, params: Params, jump, q=0.0, policy="textbook", n_lower=1_000_000, n_outer=8192,
                                   n_inner=1024, stream_lower=None, stream_outer=None, stream_inner=None, betas=None,
                                   want_q=False, want_samples=False, exercise_every=0, suboptimality_check=None):
        """Andersen-Broadie bounds of the Bermudan game under jump-diffusion (omc_price_american_bounds_jump: Merton on
        GBM, Bates on Heston scheme reference or full_truncation) -> the dict of price_american_bounds.  jump: (lambda,
        mu_j, sigma_j); q: dividend yield.  The policy is a function of the spot alone; the inner paths start at the outer
        spot (Merton) or (spot, variance) state (Bates).  Streams default to params.stream + 1 / 2 / 3.
        exercise_every: as price_american_bounds takes it.
        suboptimality_check: as price_american_bounds takes it, "off" or "payoff" ("european" is refused with -40)."""
        law = (C.byref(make_jump(jump)), float(q))
        with self._bounds_checking(suboptimality_check):
            return self._bounds("omc_price_american_bounds_jump", law, Bounds, params, policy, n_lower, n_outer, n_inner,
                                stream_lower, stream_outer, stream_inner, betas, want_q, want_samples,
                                exercise_every=exercise_every)

    def price_american_bounds_div(self, params: Params, q=0.0, dividends=(), policy="textbook", n_lower=1_000_000,
                                  n_outer=8192, n_inner=1024, stream_lower=None, stream_outer=None, stream_inner=None,
                                  betas=None, want_q=False, want_samples=False, exercise_every=0, suboptimality_check=None):
        """Andersen-Broadie bounds of the Bermudan game on a stock that pays discrete dividends
        (omc_price_american_bounds_div: GBM, or Heston scheme reference or full_truncation) -> the dict of
        price_american_bounds.  q: dividend yield; dividends: as price_american_div takes them.  Exercise at a dividend step
        earns the ex-dividend payoff.  The policy is a function of the spot alone; the inner paths start at the outer spot
        (GBM) or (spot, variance) state (Heston) and at the outer date.  Streams default to params.stream + 1 / 2 / 3.
        exercise_every: as price_american_bounds takes it.
        suboptimality_check: as price_american_bounds takes it, "off" or "payoff" ("european" is refused with -40)."""
        arr, n = dividend_array(dividends)
        with self._bounds_checking(suboptimality_check):
            return self._bounds("omc_price_american_bounds_div", (float(q), arr, n), Bounds, params, policy, n_lower, n_outer,
                                n_inner, stream_lower, stream_outer, stream_inner, betas, want_q, want_samples,
                                exercise_every=exercise_every)

    def price_barrier_bounds(self, params: Params, kind, H, monitoring="discrete", policy="textbook", n_lower=1_000_000,
                             n_outer=8192, n_inner=1024, stream_lower=None, stream_outer=None, stream_inner=None, betas=None,
                             want_q=False, want_samples=False, exercise_every=0, suboptimality_check=None):
        """Andersen-Broadie bounds of the American barrier option price_barrier quotes (omc_price_american_bounds_barrier:
        GBM, or Heston scheme reference or full_truncation; discrete monitoring) -> the dict of price_american_bounds.
        kind: a key of BARRIER_KINDS or its code.  The policy is a function of the ENCODED index (the spot where the option
        is live, the dead spot elsewhere); the inner paths start at the outer (spot, hit[, variance]) state; a knocked-out
        path stops with value 0 and an item of a dead knock-out has q = 0 and no steps.  Streams default to params.stream +
        1 / 2 / 3.
        exercise_every: as price_american_bounds takes it (monitoring stays on every step).
        suboptimality_check: as price_american_bounds takes it, "off" or "payoff" ("european" is refused with -12)."""
        law = (C.byref(make_barrier(kind, H, monitoring)),)
        with self._bounds_checking(suboptimality_check):
            return self._bounds("omc_price_american_bounds_barrier", law, Bounds, params, policy, n_lower, n_outer, n_inner,
                                stream_lower, stream_outer, stream_inner, betas, want_q, want_samples,
                                exercise_every=exercise_every)

    def price_american_basket_bounds(self, params: Params, basket: Basket, policy="textbook", n_lower=1_000_000,
                                     n_outer=8192, n_inner=1024, stream_lower=None, stream_outer=None, stream_inner=None,
                                     betas=None, want_q=False, want_samples=False, regressors="index",
                                     suboptimality_check=None):
        """Andersen-Broadie bounds of the Bermudan game on the INDEX of 1 .. 8 correlated GBM assets
        (omc_price_american_basket_bounds; arithmetic basket, best-of, worst-of) -> the dict of price_american_bounds plus
        index0, n_assets, kind.  params and basket as price_american_basket takes them; the policy is a function of the
        index alone.  Streams default to params.stream + 1 / 2 / 3.
        regressors="index+runner-up" (omc_price_american_basket_bounds_runnerup; best-of and worst-of on 2 .. 8 assets,
        policy "textbook" or "given"): the policy sees the index and the second order statistic of the weighted spots, and
        `betas` (given and returned) is [n_steps+1][8] = c0 .. c5, n, 0.  regressors="index+spot": the same entry point for
        the Asian kinds, whose second regressor is the current basket value.
        suboptimality_check: as price_american_bounds takes it, "off" or "payoff" with regressors "index" (anything else is
        refused with -40)."""
        check_runnerup(regressors, policy, int(basket.kind), int(basket.n_assets))
        entry = "omc_price_american_basket_bounds" + ("" if regressors == "index" else "_runnerup")
        with self._bounds_checking(suboptimality_check):  # (no exercise_every: the option "bounds_exercise_every" stays)
            return self._bounds(entry, (C.byref(basket),), BasketBounds, params, policy, n_lower, n_outer, n_inner,
                                stream_lower, stream_outer, stream_inner, betas, want_q, want_samples,
                                4 if regressors == "index" else 8)

    def _bounds(self, entry, law, result, params, policy, n_lower, n_outer, n_inner, stream_lower, stream_outer, stream_inner,
                betas, want_q, want_samples, cols=4, regressors=0, exercise_every=None):
        """The one call behind the price_*bounds* methods: entry(ctx, params, *law, cfg, betas, betas_out, q, samples,
        result) -- `law` are the entry point's own arguments, `result` is Bounds or BasketBounds -- with option
        "bounds_exercise_every" = exercise_every around it (None: as the context holds it)."""
        N = int(params.n_steps)
        cfg = BoundsConfig()
        cfg.regressors = regressors  # read by the Heston entry point alone
        cfg.policy = BOUND_POLICIES.get(policy, -1) if isinstance(policy, str) else int(policy)
        cfg.n_lower, cfg.n_outer, cfg.n_inner = int(n_lower), int(n_outer), int(n_inner)
        base = int(params.stream)
        cfg.stream_lower = base + 1 if stream_lower is None else int(stream_lower)
        cfg.stream_outer = base + 2 if stream_outer is None else int(stream_outer)
        cfg.stream_inner = base + 3 if stream_inner is None else int(stream_inner)
        b = None
        if betas is not None:
            b = np.ascontiguousarray(betas, np.float64)
            if b.shape != (N + 1, cols):
                raise ValueError(f"betas must have shape ({N + 1}, {cols}), got {b.shape}.")
        bo = np.zeros((N + 1, cols))
        q = np.zeros((max(int(n_outer), 0), N)) if want_q else None
        smp = np.zeros(max(int(n_outer), 0)) if want_samples else None
        tail = (b.ctypes.data if b is not None else None, bo.ctypes.data, q.ctypes.data if q is not None else None,
                smp.ctypes.data if smp is not None else None)
        out = result()
        with self._bounds_schedule(exercise_every):
            _check(self.lib, getattr(self.lib, entry)(self.handle, C.byref(params), *law, C.byref(cfg), *tail, C.byref(out)))
        base = out.bounds if result is BasketBounds else out
        d = {k: getattr(base, k) for k, _ in Bounds._fields_}
        if result is BasketBounds:
            d.update(index0=out.index0, n_assets=out.n_assets, kind=out.kind)
        d["betas"] = bo
        if want_q:
            d["q"] = q
        if want_samples:
            d["samples"] = smp
        return d

    def price_american_ols7(self, params: Params):
        """Fused pricing with regressor "ols7" (paths + omc_lsm_ols7 in the context's own matrix) -> result dict + fit."""
        res = Result()
        w, st = np.zeros(7), np.zeros(16)
        _check(self.lib, self.lib.omc_price_american_ols7(self.handle, C.byref(params), C.byref(res), w.ctypes.data,
                                                           st.ctypes.data))
        d = res.as_dict()
        d.update(weights=w, feat_mean=st[:7].copy(), feat_std=st[7:14].copy(), y_mean=float(st[14]), y_std=float(st[15]))
        return d

    def price_european(self, params: Params):
        res = Result()
        _check(self.lib, self.lib.omc_price_european(self.handle, C.byref(params), C.byref(res)))
        return res.as_dict()

    def heston_price_strikes(self, n_paths, n_steps, S0, r, T, v0, kappa, theta, xi, rho, strikes,
                             is_put=False, seed=42, stream=0, scheme=2):
        """One expiry, many strikes (the calibrator's inner call) -> (prices, stderrs)."""
        k = np.ascontiguousarray(strikes, np.float64)
        prices = np.empty_like(k)
        errs = np.empty_like(k)
        _check(self.lib, self.lib.omc_heston_price_strikes(
            self.handle, int(n_paths), int(n_steps), S0, r, T, v0, kappa, theta, xi, rho, int(seed),
            int(stream), int(scheme), k.ctypes.data, k.size, int(is_put), prices.ctypes.data,
            errs.ctypes.data))
        return prices, errs

    def heston_price_surface(self, n_paths, n_steps, S0, r, v0, kappa, theta, xi, rho, expiries, streams, strikes,
                             expiry_of, is_put=False, seed=42, scheme=2):
        """Many expiries x many strikes in one launch set (one objective evaluation of the calibrator): quote q = strike
        strikes[q] on expiry expiries[expiry_of[q]], simulated on Philox sub-stream streams[expiry_of[q]]
        -> (prices, stderrs), each quote bit-equal to its own heston_price_strikes call."""
        T = np.ascontiguousarray(expiries, np.float64)
        st = np.ascontiguousarray(streams, np.uint64)
        k = np.ascontiguousarray(strikes, np.float64)
        eo = np.ascontiguousarray(expiry_of, np.int32)
        if st.shape != T.shape or eo.shape != k.shape or T.ndim != 1 or k.ndim != 1:
            raise ValueError("expiries / streams and strikes / expiry_of must be matching 1-d arrays")
        prices = np.empty_like(k)
        errs = np.empty_like(k)
        _check(self.lib, self.lib.omc_heston_price_surface(
            self.handle, int(n_paths), int(n_steps), S0, r, v0, kappa, theta, xi, rho, int(seed), int(scheme),
            T.ctypes.data, st.ctypes.data, T.size, k.ctypes.data, eo.ctypes.data, k.size, int(is_put), prices.ctypes.data,
            errs.ctypes.data))
        return prices, errs

    def mlp_train_epoch(self, data_ptr, n_rows, batch, params_ptr, m_ptr, v_ptr, step, lr, dropout, seed,
                        hidden=64, layers=2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-5,
                        shuffle_key=0):
        """One epoch of the fused 7->64->64->1 trainer on device pointers -> (mean loss, new step).
        shuffle_key != 0: rows are visited in the keyed pseudo-random permutation."""
        st = C.c_int64(int(step))
        loss = C.c_double(0.0)
        _check(self.lib, self.lib.omc_mlp_train_epoch(
            self.handle, int(data_ptr), int(n_rows), int(batch), int(hidden), int(layers), int(params_ptr),
            int(m_ptr), int(v_ptr), C.byref(st), float(lr), float(beta1), float(beta2), float(eps),
            float(weight_decay), float(dropout), int(seed), int(shuffle_key), C.byref(loss)))
        return loss.value, st.value

    # -- the NN regressor sharded over ranks (include/omc.h; host logic in nn_dist.py)
    def nn_half_counts(self, S_ptr, ld, n_paths, n_steps, K, is_put):
        """-> int64 [(n_steps - 1), 2]: in-the-money paths per step (index n_steps - 1 - t) in the first / second half
        of the rank's columns."""
        out = np.zeros((max(int(n_steps) - 1, 0), 2), np.int64)
        _check(self.lib, self.lib.omc_nn_half_counts(self.handle, int(S_ptr), int(ld), int(n_paths), int(n_steps), float(K),
                                                     int(bool(is_put)), out.ctypes.data))
        return out

    def mlp_shard_epoch(self, data_ptr, n_rows_local, rows_global, batch, shuffle_key, gstart, lstart, data_epoch_ptr,
                        drop_pos_ptr, segs_per_step=0):
        """This rank's rows of the epoch, gathered in epoch order -> step_off (int64 [steps + 1], host)."""
        g = np.ascontiguousarray(gstart, np.int64)
        l_ = np.ascontiguousarray(lstart, np.int64)
        assert g.size == l_.size + 1
        steps = (int(rows_global) + int(batch) - 1) // int(batch)
        so = np.zeros(steps + 1, np.int64)
        _check(self.lib, self.lib.omc_mlp_shard_epoch(
            self.handle, int(data_ptr) if n_rows_local else None, int(n_rows_local), int(rows_global), int(batch),
            int(shuffle_key), g.ctypes.data, l_.ctypes.data, int(l_.size), int(segs_per_step),
            int(data_epoch_ptr) if n_rows_local else None,
            int(drop_pos_ptr) if n_rows_local else None, so.ctypes.data))
        return so

    def mlp_train_epoch_sharded(self, data_epoch_ptr, n_rows_local, rows_global, batch, params_ptr, m_ptr, v_ptr, step, lr,
                                dropout, seed, step_off, drop_pos_ptr, hidden=64, layers=2, beta1=0.9, beta2=0.999,
                                eps=1e-8, weight_decay=1e-5):
        """One epoch of the job's training on this rank's rows -> (the job's mean loss, new step)."""
        st = C.c_int64(int(step))
        loss = C.c_double(0.0)
        so = np.ascontiguousarray(step_off, np.int64)
        _check(self.lib, self.lib.omc_mlp_train_epoch_sharded(
            self.handle, int(data_epoch_ptr) if n_rows_local else None, int(n_rows_local), int(rows_global), int(batch),
            int(hidden), int(layers), int(params_ptr), int(m_ptr), int(v_ptr), C.byref(st), float(lr), float(beta1),
            float(beta2), float(eps), float(weight_decay), float(dropout), int(seed), so.ctypes.data,
            int(drop_pos_ptr) if n_rows_local else None, C.byref(loss)))
        return loss.value, st.value

    def mlp_train_epoch_batch(self, jobs, hidden, layers, dropout, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-5):
        """One epoch for every network of `jobs` (list of dicts: data_ptr, n_rows, batch, params_ptr, m_ptr, v_ptr,
        step, lr, seed, shuffle_key), all of shape hidden x layers, side by side -> [(mean_loss, new_step), ...]."""
        n = len(jobs)
        arr = (MlpJob * n)()
        for a, j in zip(arr, jobs):
            a.data, a.n_rows, a.batch = int(j["data_ptr"]), int(j["n_rows"]), int(j["batch"])
            a.params, a.adam_m, a.adam_v = int(j["params_ptr"]), int(j["m_ptr"]), int(j["v_ptr"])
            a.step, a.lr = int(j["step"]), float(j["lr"])
            a.seed, a.shuffle_key = int(j["seed"]) & (2**64 - 1), int(j["shuffle_key"]) & (2**64 - 1)
        _check(self.lib, self.lib.omc_mlp_train_epoch_batch(self.handle, arr, n, int(hidden), int(layers), float(beta1),
                                                            float(beta2), float(eps), float(weight_decay), float(dropout)))
        return [(a.mean_loss, a.step) for a in arr]

    def lsm_apply_mlp(self, S_ptr, ld, n_paths, n_steps, K, r, T, is_put, params_ptr, feat_mean, feat_std,
                      y_mean, y_std, dropout, seed, want_state=False, hidden=64, layers=2, col_bases=None):
        """Pass 2 of the NN flow on a device path matrix -> result dict (+ sx, tex if want_state).
        col_bases = (base0, base1): the matrix is one rank's shard (omc_lsm_apply_mlp_shard)."""
        fm = np.ascontiguousarray(feat_mean, np.float64)
        fs = np.ascontiguousarray(feat_std, np.float64)
        assert fm.size == 7 and fs.size == 7
        res = Result()
        sx = np.empty(n_paths, np.float32) if want_state else None
        tex = np.empty(n_paths, np.int32) if want_state else None
        b0, b1 = (0, int(n_paths) // 2) if col_bases is None else (int(col_bases[0]), int(col_bases[1]))
        _check(self.lib, self.lib.omc_lsm_apply_mlp_shard(
            self.handle, int(S_ptr), int(ld), int(n_paths), int(n_steps), float(K), float(r), float(T),
            int(bool(is_put)), int(hidden), int(layers), int(params_ptr), fm.ctypes.data, fs.ctypes.data,
            float(y_mean), float(y_std), float(dropout), int(seed), C.byref(res),
            sx.ctypes.data if want_state else None, tex.ctypes.data if want_state else None, b0, b1))
        out = res.as_dict()
        if want_state:
            out["sx"], out["tex"] = sx, tex
        return out

    def nn_build_rows(self, S_ptr, ld, n_paths, n_steps, K, r, T, is_put, data_ptr=None, cap_rows=0):
        """Pass 1 of the NN flow from a device path matrix.  data_ptr None -> row count only;
        else -> (rows, feat_mean[7], feat_std[7], y_mean, y_std) with the rows written to data_ptr."""
        n = C.c_int64(0)
        st = np.zeros(16)
        _check(self.lib, self.lib.omc_nn_build_rows(
            self.handle, int(S_ptr), int(ld), int(n_paths), int(n_steps), float(K), float(r), float(T),
            int(bool(is_put)), int(data_ptr) if data_ptr else None, int(cap_rows), C.byref(n), st.ctypes.data))
        if not data_ptr:
            return n.value
        return n.value, st[:7].copy(), st[7:14].copy(), float(st[14]), float(st[15])

    def nn_feature_stats(self, x_ptr, t_ptr, y_ptr, n_rows, T, dt):
        """-> (means[7], variances[7]) of [x, x^2, x^3, max(x-1,0), s, x*s, y] over device rows."""
        out = np.zeros(16)
        _check(self.lib, self.lib.omc_nn_feature_stats(self.handle, int(x_ptr), int(t_ptr), int(y_ptr),
                                                       int(n_rows), float(T), float(dt), out.ctypes.data))
        return out[:7].copy(), out[8:15].copy()

    def mlp_dropout_masks(self, variant, hidden, layers, n_rows, step, seed, dropout, keys=None):
        """keep (True) / drop of every hidden activation as kernel `variant` draws it -> bool [layers, n_rows, hidden]
        (variant 0: pass 2, keys = path columns, step = time step; 1 .. 4: omc_mlp_train_variant)."""
        out = np.zeros((int(layers), int(n_rows), int(hidden)), np.uint8)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint32)
        assert k is None or k.size == n_rows
        _check(self.lib, self.lib.omc_mlp_dropout_masks(self.handle, int(variant), int(hidden), int(layers), int(n_rows),
                                                         k.ctypes.data if k is not None else None, int(step),
                                                         int(seed) & (2 ** 64 - 1), float(dropout), out.ctypes.data))
        return out.astype(bool)

    def mlp_shuffle_indices(self, n_rows, shuffle_key, out_ptr):
        _check(self.lib, self.lib.omc_mlp_shuffle_indices(self.handle, int(n_rows), int(shuffle_key), int(out_ptr)))

    # -- many small pricings as one set of launches (all share model/semantics/antithetic)
    MAX_BATCH = 65535

    def _batch(self, fn, params_list):
        out = []
        for lo in range(0, len(params_list), self.MAX_BATCH):
            chunk = params_list[lo:lo + self.MAX_BATCH]
            n = len(chunk)
            arr = (Params * n)(*chunk)
            res = (Result * n)()
            _check(self.lib, fn(self.handle, arr, n, res))
            out.extend(r.as_dict() for r in res)
        return out

    def price_american_seq(self, params_list):
        """n pricings back to back on the stream, one wait at the end -> list of result dicts."""
        plist = list(params_list)
        n = len(plist)
        arr = (Params * n)(*plist)
        res = (Result * n)()
        _check(self.lib, self.lib.omc_price_american_seq(self.handle, arr, n, res))
        return [r.as_dict() for r in res]

    def seq_step_width(self, params_list) -> int:
        """How many pricings of this sequence share one launch per time step (per-step flows; 1 = none)."""
        plist = list(params_list)
        arr = (Params * len(plist))(*plist)
        return int(self.lib.omc_seq_step_width(self.handle, arr, len(plist)))

    def seq_group_width(self, params_list) -> int:
        """How many pricings of the run that starts this sequence share their small launches (two-pass flow; 1 = none)."""
        plist = list(params_list)
        arr = (Params * len(plist))(*plist)
        return int(self.lib.omc_seq_group_width(self.handle, arr, len(plist)))

    def price_american_chain(self, params: Params, strikes, is_put=True, want_betas=False, exercise_every=0):
        """A whole chain of one expiry from one set of paths (omc_price_american_chain) -> (list of result dicts, info dict).
        strikes: the entries' strikes; is_put: one flag for all or one per strike; params.K / params.is_put are ignored.
        Entry i carries the bits of price_american(params with strikes[i], is_put[i]); want_betas adds its fits
        [n_steps+1][4] as "betas".  exercise_every: one schedule for all or one per strike (ChainEntry); an entry with k >= 2 is
        the Bermudan quote, its fits zero at every unscheduled date."""
        ks = [float(k) for k in strikes]
        n = len(ks)
        every = [int(exercise_every)] * n if isinstance(exercise_every, (int, np.integer)) else [int(k) for k in exercise_every]
        if len(every) != n:
            raise ValueError("one exercise_every per strike.")
        sides = [int(bool(is_put))] * n if isinstance(is_put, (bool, int, np.integer)) else [int(bool(s)) for s in is_put]
        if len(sides) != n:
            raise ValueError("one side per strike.")
        ent = (ChainEntry * max(n, 1))()
        for i in range(n):
            ent[i].K, ent[i].is_put, ent[i].exercise_every = ks[i], sides[i], every[i]
        res = (Result * max(n, 1))()
        info = ChainInfo()
        N = int(params.n_steps)
        bo = np.zeros((max(n, 1), N + 1, 4)) if want_betas else None
        _check(self.lib, self.lib.omc_price_american_chain(self.handle, C.byref(params), ent, n, res,
                                                            bo.ctypes.data if bo is not None else None, C.byref(info)))
        out = [res[i].as_dict() for i in range(n)]
        if want_betas:
            for i in range(n):
                out[i]["betas"] = bo[i]
        return out, {k: getattr(info, k) for k, _ in ChainInfo._fields_ if k != "reserved"}

    def price_american_chain_bounds(self, params: Params, strikes, is_put=True, policy="textbook", n_lower=1_000_000,
                                    n_outer=8192, n_inner=1024, stream_lower=None, stream_outer=None, stream_inner=None,
                                    betas=None, want_q=False, want_samples=False, exercise_every=0):
        """Andersen-Broadie bounds of every quote of a chain from one set of fresh paths (omc_price_american_chain_bounds;
        GBM, or Heston scheme reference or full_truncation) -> (list of the dicts of price_american_bounds, info dict).
        strikes, is_put and exercise_every as price_american_chain takes them (an entry with exercise_every != 0 is refused
        with -44); params.K / params.is_put are ignored.  policy and the sizes as price_american_bounds; betas: the tables
        of policy "given", [n][n_steps+1][4].  Entry i carries the bits of its own price_american_bounds /
        price_american_bounds_heston call in betas, lower, se_lower, n_exercised_lower and inner_path_steps -- and in q,
        samples, upper and se_upper while n_inner <= 128; beyond, those differ by the order of float64 sums.  Streams default
        to params.stream + 1 / 2 / 3.  info: inner_path_steps_simulated, n_groups, entries_per_group and the phase times."""
        ks = [float(k) for k in strikes]
        n = len(ks)
        every = [int(exercise_every)] * n if isinstance(exercise_every, (int, np.integer)) else [int(k) for k in exercise_every]
        if len(every) != n:
            raise ValueError("one exercise_every per strike.")
        sides = [int(bool(is_put))] * n if isinstance(is_put, (bool, int, np.integer)) else [int(bool(s)) for s in is_put]
        if len(sides) != n:
            raise ValueError("one side per strike.")
        ent = (ChainEntry * max(n, 1))()
        for i in range(n):
            ent[i].K, ent[i].is_put, ent[i].exercise_every = ks[i], sides[i], every[i]
        N, m, no = int(params.n_steps), max(n, 1), max(int(n_outer), 0)
        cfg = BoundsConfig()
        cfg.policy = BOUND_POLICIES.get(policy, -1) if isinstance(policy, str) else int(policy)
        cfg.n_lower, cfg.n_outer, cfg.n_inner = int(n_lower), int(n_outer), int(n_inner)
        base = int(params.stream)
        cfg.stream_lower = base + 1 if stream_lower is None else int(stream_lower)
        cfg.stream_outer = base + 2 if stream_outer is None else int(stream_outer)
        cfg.stream_inner = base + 3 if stream_inner is None else int(stream_inner)
        b = None
        if betas is not None:
            b = np.ascontiguousarray(betas, np.float64)
            if b.shape != (n, N + 1, 4):
                raise ValueError(f"betas must have shape ({n}, {N + 1}, 4), got {b.shape}.")
        bo = np.zeros((m, N + 1, 4))
        q = np.zeros((m, no, N)) if want_q else None
        smp = np.zeros((m, no)) if want_samples else None
        res = (Bounds * m)()
        info = ChainBoundsInfo()
        _check(self.lib, self.lib.omc_price_american_chain_bounds(
            self.handle, C.byref(params), ent, n, C.byref(cfg), b.ctypes.data if b is not None else None, bo.ctypes.data,
            q.ctypes.data if q is not None else None, smp.ctypes.data if smp is not None else None, res, C.byref(info)))
        outs = []
        for i in range(n):
            d = {k: getattr(res[i], k) for k, _ in Bounds._fields_}
            d["betas"] = bo[i]
            if want_q:
                d["q"] = q[i]
            if want_samples:
                d["samples"] = smp[i]
            outs.append(d)
        return outs, {k: getattr(info, k) for k, _ in ChainBoundsInfo._fields_}

    def price_american_chain_greeks(self, params: Params, strikes, is_put=True, bump=0.01, betas=None, want_betas=False,
                                    exercise_every=0):
        """Frozen-policy pathwise Greeks of every quote of a chain from one set of paths (omc_price_american_chain_greeks) ->
        (list of the dicts of price_american_greeks, info dict).  strikes, is_put and exercise_every as price_american_chain
        takes them; params.K / params.is_put are ignored.  An American entry carries the bits of its own
        price_american_greeks call; a Bermudan entry (exercise_every >= 2) those of that call with its masked policy given
        (but sum_nitm).  betas: one given policy per entry, [n][n_steps+1][4]; want_betas adds the policy used as "betas".
        info: folded, n_groups, n_sweep_launches, entries_per_launch and the phase times."""
        ks = [float(k) for k in strikes]
        n = len(ks)
        every = [int(exercise_every)] * n if isinstance(exercise_every, (int, np.integer)) else [int(k) for k in exercise_every]
        if len(every) != n:
            raise ValueError("one exercise_every per strike.")
        sides = [int(bool(is_put))] * n if isinstance(is_put, (bool, int, np.integer)) else [int(bool(s)) for s in is_put]
        if len(sides) != n:
            raise ValueError("one side per strike.")
        ent = (ChainEntry * max(n, 1))()
        for i in range(n):
            ent[i].K, ent[i].is_put, ent[i].exercise_every = ks[i], sides[i], every[i]
        N, m = int(params.n_steps), max(n, 1)
        b = None
        if betas is not None:
            b = np.ascontiguousarray(betas, np.float64)
            if b.shape != (n, N + 1, 4):
                raise ValueError(f"betas must have shape ({n}, {N + 1}, 4), got {b.shape}.")
        bo = np.zeros((m, N + 1, 4)) if want_betas else None
        res = (Greeks * m)()
        info = ChainGreeksInfo()
        _check(self.lib, self.lib.omc_price_american_chain_greeks(
            self.handle, C.byref(params), ent, n, float(bump), b.ctypes.data if b is not None else None,
            bo.ctypes.data if bo is not None else None, res, C.byref(info)))
        outs = [_with_base(res[i]) for i in range(n)]
        if want_betas:
            for i in range(n):
                outs[i]["betas"] = bo[i]
        return outs, {k: getattr(info, k) for k, _ in ChainGreeksInfo._fields_}

    def chain_width(self, params: Params, n: int) -> int:
        """Entries per fused launch of a chain of n entries like params (omc_chain_width; 1 = unfused route, 0 = invalid)."""
        return int(self.lib.omc_chain_width(self.handle, C.byref(params), int(n)))

    def price_american_batch(self, params_list):
        return self._batch(self.lib.omc_price_american_batch, list(params_list))

    def price_american_contnet_batch(self, params_list, nn_hidden=32, nn_epochs=10, nn_lr=1e-3, nn_seeds=0):
        """Many pricings with the v1 / v2 regressor (fresh ContNet per step) as one set of launches.
        nn_seeds: one seed for all, or one per problem."""
        plist = list(params_list)
        n = len(plist)
        seeds = [int(nn_seeds)] * n if isinstance(nn_seeds, (int, np.integer)) else [int(x) for x in nn_seeds]
        assert len(seeds) == n
        out = []
        for lo in range(0, n, self.MAX_BATCH):
            chunk = plist[lo:lo + self.MAX_BATCH]
            k = len(chunk)
            arr = (Params * k)(*chunk)
            sd = (C.c_uint64 * k)(*[x & (2**64 - 1) for x in seeds[lo:lo + k]])
            res = (Result * k)()
            _check(self.lib, self.lib.omc_price_american_contnet_batch(self.handle, arr, k, int(nn_hidden), int(nn_epochs),
                                                                       float(nn_lr), sd, res))
            out.extend(r.as_dict() for r in res)
        return out

    def price_european_batch(self, params_list):
        return self._batch(self.lib.omc_price_european_batch, list(params_list))


def make_params(model="gbm", is_put=True, semantics="reference", antithetic=True,
                heston_scheme="reference", n_paths=0, n_steps=0, S0=100.0, K=100.0, r=0.05,
                sigma=0.2, T=1.0, v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7, seed=42,
                stream=0, pair_offset=0) -> Params:
    p = Params()
    p.model = MODELS[model.lower()]
    p.is_put = int(bool(is_put))
    p.semantics = SEMANTICS[semantics]
    p.antithetic = int(bool(antithetic))
    p.heston_scheme = HESTON_SCHEMES[heston_scheme] if isinstance(heston_scheme, str) else int(heston_scheme)
    p.n_steps = int(n_steps)
    p.n_paths = int(n_paths)
    p.S0, p.K, p.r, p.sigma, p.T = float(S0), float(K), float(r), float(sigma or 0.0), float(T)
    p.v0, p.kappa, p.theta, p.xi, p.rho = float(v0), float(kappa), float(theta), float(xi), float(rho)
    p.seed, p.stream, p.pair_offset = int(seed), int(stream), int(pair_offset)
    return p


_default_ctx = {}
_ctx_lock = threading.Lock()


def resolve_device(device=None) -> int:
    """Which HIP device a call without an explicit `device` uses.  Default 0.  OMC_DEVICE=<k> picks device k;
    OMC_DEVICE=auto spreads PROCESSES over the node's GPUs by pid -- the reference's UIs fan the spot values of a curve
    job over a spawn pool (options_model_2_ui.py:87-133, options_model_3.py:1043-1056): with `auto` those workers,
    whose pids are consecutive, land on different GPUs without a change to the caller."""
    if device is not None:
        return int(device)
    env = os.environ.get("OMC_DEVICE", "").strip().lower()
    if not env:
        return 0
    if env == "auto":
        n = device_count()
        return os.getpid() % n if n > 0 else 0
    return int(env)


def default_context(device=None) -> Context:
    """Lazily created per (process, device) -- safe under spawn'ed worker pools."""
    device = resolve_device(device)
    key = (os.getpid(), device)
    with _ctx_lock:
        ctx = _default_ctx.get(key)
        if ctx is None:
            ctx = Context(device)
            _default_ctx[key] = ctx
        return ctx


_pools = {}


def context_pool(n: int, device: int = 0) -> list:
    """n DEDICATED contexts on one device (own stream and workspaces each; never default_context(), which other
    code of the process may be using at the same time -- an omc_ctx is not thread-safe): for work made of many
    small, latency-bound pricings -- the per-step network flow of the v1 / v2 curves -- which overlap on the GPU
    when issued from several host threads (ctypes releases the GIL during a call)."""
    key = (os.getpid(), device)
    with _ctx_lock:
        pool = _pools.setdefault(key, [])
        while len(pool) < n:
            pool.append((Context(device), threading.Lock()))
        return pool[:n]


def map_contexts(fn, items, workers: int | None = None, device: int = 0) -> list:
    """[fn(ctx, item) for item in items], in order, run by `workers` host threads with one context each
    (OMC_CURVE_STREAMS, default 8; 1 = plain loop on the default context).  Every pool context is used under
    its own lock, so two map_contexts calls running at once (two threads of the caller) share the pool safely."""
    items = list(items)
    if workers is None:
        workers = int(os.environ.get("OMC_CURVE_STREAMS", "8"))
    workers = max(1, min(int(workers), len(items)))
    if workers == 1:
        ctx = default_context(device)
        return [fn(ctx, it) for it in items]
    from concurrent.futures import ThreadPoolExecutor
    pool = context_pool(workers, device)

    def one(args):
        i, it = args
        ctx, lock = pool[i % workers]
        with lock:
            return fn(ctx, it)

    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(one, enumerate(items)))
