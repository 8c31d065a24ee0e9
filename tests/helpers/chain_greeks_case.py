"""What tests/test_gpu_chain_greeks.py and tests/test_gpu_chain_greeks_fuzz.py share: the fields of an entry compared bit for
bit, the matrix the chain stores, and the restatement of an entry's route on it (tests/helpers/chain_greeks_ref.py).  TEST
INFRASTRUCTURE ONLY."""
import numpy as np

from helpers import chain_greeks_ref as cg
from helpers import greeks_check as gk
from oracle import cpu as orc

BASE = ("price", "sum", "sumsq", "std", "zero_prob", "n_paths", "n_exercised", "n_zero", "sum_nitm", "folded")
GREEKS = ("delta", "gamma", "vega", "rho", "theta", "se_delta", "se_gamma", "se_vega", "se_rho", "se_theta", "bump", "price_up",
          "price_down", "n_exercised_up", "n_exercised_down")


def bits(x):
    return np.float64(x).tobytes() if isinstance(x, float) else x


def same(a, b, what, skip=()):
    """every field but the times, bit for bit (NaN equals NaN of the same bits)"""
    for k in BASE + GREEKS:
        if k not in skip:
            assert bits(a[k]) == bits(b[k]), (what, k, a[k], b[k])
    if "betas" in a and "betas" in b:
        assert np.array_equal(a["betas"], b["betas"]), (what, "betas")


def device_matrix(c, p, folded):
    d = gk.stored_half(c, p) if folded else gk.stored(c, p)
    S = d.to_host()
    d.free()
    return S


def restate(S, p, K, put, k, betas, h, folded):
    cK = None
    if folded:
        c0, g = orc.fold_constants(p.S0, K, p.r, p.sigma, p.T, p.n_steps)
        cK = orc.fold_table(p.n_steps, c0, g)
    return cg.view_greeks(S, K, p.r, p.T, put, betas, p.S0, p.sigma, h=h, every=k, cK=cK, gbm=p.model == 0)
