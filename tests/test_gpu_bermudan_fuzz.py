"""A seeded random sweep of the Bermudan chain entries (omc_chain_entry::exercise_every): random N in 1 .. 70, schedules,
ragged path counts, both storages, GBM and Heston, pair offsets (tests/helpers/bermudan_ref.py: fuzz_cases), each against
its restatement on the device's own matrix with the comparisons of tests/test_gpu_bermudan.py.
OMC_FUZZ_SCALE multiplies the case count, OMC_FUZZ_SEED shifts the seed (the pattern of tests/test_gpu_fuzz.py)."""
import os

import numpy as np
import pytest

from helpers import bermudan_ref as br
from options_model_amd import _ffi

pytestmark = pytest.mark.gpu

_SCALE = int(os.environ.get("OMC_FUZZ_SCALE", "1"))
_SHIFT = int(os.environ.get("OMC_FUZZ_SEED", "0"))
CASES = br.fuzz_cases(8 * _SCALE, 232323 + _SHIFT)


@pytest.fixture
def cctx(ctx):
    yield ctx
    ctx.set_option("fold_antithetic", 1)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_random_bermudan_entry_equals_its_restatement(cctx, i):
    from test_gpu_bermudan import device_matrix
    c = CASES[i]
    cctx.set_option("fold_antithetic", 2 if c["folded"] else 0)
    kw = dict(br.HESTON, model="heston", heston_scheme=c["scheme"]) if c["model"] == "heston" else {}
    p = _ffi.make_params(semantics="two_pass", n_paths=c["M"], n_steps=c["N"], S0=c["S0"], K=c["K"], r=c["r"], sigma=c["sigma"],
                         T=c["T"], seed=c["seed"], stream=c["stream"], pair_offset=c["pair_offset"], is_put=c["is_put"], **kw)
    outs, info = cctx.price_american_chain(p, [c["K"]] * 2, c["is_put"], want_betas=True, exercise_every=[0, c["k"]])
    assert info["folded"] == int(c["folded"]) and info["fused"] == 0
    am, o = outs
    for key in ("price", "sum", "sumsq", "n_exercised", "n_zero", "sum_nitm"):
        assert am[key] == cctx.price_american(p)[key], (i, key)
    ref = br.reference(c, device_matrix(cctx, p, c["folded"]))
    br.assert_agrees(o, ref, (i, c))
    mask = br.schedule(c["N"], c["k"])
    assert np.array_equal(o["betas"][mask], am["betas"][mask]) and not o["betas"][~mask].any(), i
    assert o["sum_nitm"] == int(am["betas"][mask, 3].sum()), i
    if c["k"] >= c["N"]:
        assert o["n_exercised"] == 0
