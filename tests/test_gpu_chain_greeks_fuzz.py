"""A seeded random sweep of the chain's Greeks (omc_price_american_chain_greeks): 1 .. 70 steps, ragged even path counts on
both storages, 1 .. 20 entries with random sides, strikes and schedules 0 .. N + 3, pair offsets, bumps 0.001 .. 0.5, r = 0
(tests/helpers/chain_greeks_ref.py: fuzz_cases; tests/test_chain_greeks_cpu.py checks without a GPU that the first eight are
free of ties).  Every entry against the restatement of the view's route on the device's own matrix, every American entry
against its own omc_price_american_greeks call bit for bit.
OMC_FUZZ_SCALE multiplies the case count, OMC_FUZZ_SEED shifts the seed (the pattern of tests/test_gpu_fuzz.py)."""
import os

import numpy as np
import pytest

from helpers import chain_greeks_ref as cg
from helpers import greeks_check as gk
from helpers.chain_greeks_case import device_matrix, restate
from helpers.chain_greeks_case import same as _same
from options_model_amd import _ffi

pytestmark = pytest.mark.gpu

_SCALE = int(os.environ.get("OMC_FUZZ_SCALE", "1"))
_SHIFT = int(os.environ.get("OMC_FUZZ_SEED", "0"))
CASES = cg.fuzz_cases(8 * _SCALE, 353535 + _SHIFT)


@pytest.fixture
def cctx(ctx):
    yield ctx
    ctx.set_option("fold_antithetic", 1)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_random_chain_equals_its_restatement_and_its_single_calls(cctx, i):
    c = CASES[i]
    cctx.set_option("fold_antithetic", 2 if c["folded"] else 0)
    kw = dict(cg.HESTON, model="heston", heston_scheme=c["scheme"]) if c["model"] == "heston" else {}

    def params(K, put):
        return _ffi.make_params(semantics="two_pass", n_paths=c["M"], n_steps=c["N"], S0=c["S0"], K=K, r=c["r"], sigma=c["sigma"],
                                T=c["T"], seed=c["seed"], stream=c["stream"], pair_offset=c["pair_offset"], is_put=put, **kw)

    p = params(c["strikes"][0], c["puts"][0])
    outs, info = cctx.price_american_chain_greeks(p, c["strikes"], c["puts"], bump=c["bump"], want_betas=True,
                                                  exercise_every=c["every"])
    assert info["folded"] == int(c["folded"]) and info["n_groups"] == (len(outs) + 15) // 16
    S = device_matrix(cctx, p, c["folded"])
    for j, (o, K, put, k) in enumerate(zip(outs, c["strikes"], c["puts"], c["every"])):
        q = params(K, put)
        gk.agrees(o, restate(S, p, K, put, k, o["betas"], c["bump"], c["folded"]), q)
        if k < 2:
            _same(o, cctx.price_american_greeks(q, bump=c["bump"], want_betas=True), (i, j, K, put, k))
        else:
            mask = np.zeros(c["N"] + 1, bool)
            mask[cg.view_dates(c["N"], k)[1:-1]] = True
            assert not o["betas"][~mask].any(), (i, j)
            if k >= c["N"]:
                assert o["n_exercised"] == 0
