"""Seeded random sweep of omc_price_american_div: shapes 2 .. 30,000 paths x 1 .. 64 steps, 0 .. 6 dividends of random
kind, time and size, a yield of either sign, GBM and the three Heston schemes.  Every case runs the two device checks of
tests/test_gpu_dividends.py: the matrix against tests/helpers/dividend_ref.apply on the vanilla device matrix, and the
price against the C oracle's two-pass flow on the device's own matrix.  OMC_FUZZ_SCALE multiplies the number of cases
and OMC_FUZZ_SEED shifts the seed, as in tests/test_gpu_fuzz.py; the generator is tested on the CPU
(tests/test_dividends_cpu.py)."""
import os

import numpy as np
import pytest

import test_gpu_dividends as td

pytestmark = pytest.mark.gpu

_SCALE = int(os.environ.get("OMC_FUZZ_SCALE", "1"))
_SHIFT = int(os.environ.get("OMC_FUZZ_SEED", "0"))
SEED = 20261017
N_CASES = 24

_MODELS = [("gbm", 0), ("heston", 0), ("heston", 1), ("heston", 2)]
# the first cases of every draw are dealt the edges, whatever the seed: (pairs per thread, steps, dividends); the second
# one is a single pair
_EDGES = [(4, 64, 6), (1, 1, 1), (2, 33, 0), (4, 7, 3), (1, 2, 6), (2, 50, 2), (4, 4, 1), (1, 5, 4)]


def vec_of(c):
    """pairs per thread the generator picks for the case's matrix (leading dimension = n_paths)"""
    P = c["M"] // 2
    return 4 if P % 4 == 0 else 2 if P % 2 == 0 else 1


def cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        vec, N, nd = _EDGES[i] if i < len(_EDGES) else (int(rng.choice([1, 2, 4])), int(rng.integers(1, 65)), int(rng.integers(0, 7)))
        if vec == 4:
            P = 4 * int(rng.integers(1, 3751))
        elif vec == 2:
            P = 4 * int(rng.integers(0, 3750)) + 2
        else:
            P = 1 if i == 1 else 2 * int(rng.integers(0, 7500)) + 1
        model, scheme = _MODELS[i % 4] if i < 8 else _MODELS[int(rng.integers(0, 4))]
        T = float(rng.choice([0.25, 1.0, 2.0]))
        s0 = float(rng.uniform(60.0, 140.0))
        divs = []
        for _ in range(nd):
            t = float(rng.uniform(1e-6, T)) if rng.random() < 0.8 else T
            if rng.random() < 0.5:
                divs.append((t, float(rng.uniform(0.0, 0.04) * s0), "cash"))
            else:
                divs.append((t, float(rng.uniform(0.0, 0.05)), "proportional"))
        q = float(rng.uniform(0.005, 0.06)) * (-1.0 if i % 5 == 2 else 1.0)
        out.append(dict(model=model, scheme=scheme, M=2 * P, N=N, divs=divs, q=q, is_put=bool(rng.integers(0, 2)), S0=s0,
                        K=s0 * float(rng.uniform(0.9, 1.1)), r=float(rng.choice([0.0, 0.03, 0.08])),
                        sigma=float(rng.choice([0.1, 0.2, 0.45])), T=T, seed=int(rng.integers(1, 2 ** 31)),
                        stream=int(rng.integers(0, 5)), off=int(rng.choice([0, 0, 12345, 2 ** 33 + 7]))))
    return out


def params(c):
    s2 = c["sigma"] ** 2
    return td.params(c["model"], c["scheme"], is_put=c["is_put"], M=c["M"], N=c["N"], seed=c["seed"], stream=c["stream"],
                     pair_offset=c["off"], S0=c["S0"], K=c["K"], r=c["r"], sigma=c["sigma"], T=c["T"], v0=s2, theta=s2)


@pytest.mark.parametrize("case", cases(N_CASES * _SCALE, SEED + _SHIFT),
                         ids=lambda c: f"{c['model']}{c['scheme']}-{c['M']}x{c['N']}-{len(c['divs'])}div")
def test_dividend_pricing_sweep(ctx, case):
    c = case
    p = params(c)
    out, S = td.priced(ctx, p, c["q"], c["divs"])
    _, has = td.check_matrix(ctx, p, c["q"], c["divs"], S, c["model"])
    assert out["n_div_steps"] == int(has.sum()) and out["folded"] == 0
    td.check_price(out, S, p)
