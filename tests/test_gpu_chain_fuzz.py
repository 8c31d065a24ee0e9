"""A seeded random sweep of omc_price_american_chain: every entry of every random chain (tests/helpers/chain_cases.py)
against its own omc_price_american call, bit for bit -- results and fits, folded and full storage, fused and unfused.
OMC_FUZZ_SCALE multiplies the case count, OMC_FUZZ_SEED shifts the seed (the pattern of tests/test_gpu_fuzz.py)."""
import os

import numpy as np
import pytest

from helpers import chain_cases as cc

pytestmark = pytest.mark.gpu

_SCALE = int(os.environ.get("OMC_FUZZ_SCALE", "1"))
_SHIFT = int(os.environ.get("OMC_FUZZ_SEED", "0"))
KEYS = ("price", "sum", "sumsq", "std", "zero_prob", "n_exercised", "n_zero", "sum_nitm", "n_paths", "folded")
CASES = cc.chain_cases(16 * _SCALE, 171717 + _SHIFT)


@pytest.fixture
def cctx(ctx):
    yield ctx
    ctx.set_option("chain_fused", 0)
    ctx.set_option("chain_k", -1)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_random_chain_equals_its_single_calls(cctx, i):
    from options_model_amd import _ffi
    c = CASES[i]

    def params(K, put):
        return _ffi.make_params(semantics="two_pass", n_paths=c["M"], n_steps=c["N"], S0=c["S0"], K=K, r=c["r"],
                                sigma=c["sigma"], T=c["T"], seed=c["seed"], is_put=put)

    singles = [cctx.price_american(params(K, put)) for K, put in zip(c["strikes"], c["sides"])]
    fits = [cctx.price_american_greeks(params(K, put), want_betas=True)["betas"] for K, put in zip(c["strikes"], c["sides"])]
    cctx.set_option("chain_k", c["chain_k"])
    for fused in (1, 0):
        cctx.set_option("chain_fused", fused)
        outs, info = cctx.price_american_chain(params(1.0, True), c["strikes"], c["sides"], want_betas=True)
        assert info["folded"] == int(cc.is_folded(c)) and info["fused"] == (fused if cc.is_folded(c) else 0)
        for o, s, b in zip(outs, singles, fits):
            for k in KEYS:
                assert o[k] == s[k], (i, fused, k, o[k], s[k])
            assert np.array_equal(o["betas"], b), (i, fused)
