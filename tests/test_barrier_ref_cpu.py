"""CPU suite: the barrier references (tests/helpers/barrier_ref.py) -- closed forms, the Brownian-bridge Monte Carlo,
the encoder -- and the v2 compat stub of ExoticOptionPricer called as the reference's main() calls it."""
import math

import numpy as np
import pytest

from helpers import barrier_ref as br

S0, R, SIG, T = 100.0, 0.05, 0.2, 1.0
CASES = [(kind, is_put) for kind in br.KINDS for is_put in (True, False)]


def _H(kind, far=False):
    if kind.startswith("down"):
        return 1e-6 * S0 if far else 85.0
    return 1e6 * S0 if far else 120.0


@pytest.mark.parametrize("K", [90.0, 100.0, 115.0])
@pytest.mark.parametrize("down", [True, False])
@pytest.mark.parametrize("is_put", [True, False])
def test_in_plus_out_is_black_scholes(K, down, is_put):
    H = 85.0 if down else 120.0
    pre = "down" if down else "up"
    v_in = br.closed_form(pre + "-and-in", is_put, S0, K, H, R, SIG, T)
    v_out = br.closed_form(pre + "-and-out", is_put, S0, K, H, R, SIG, T)
    bs = br.black_scholes(S0, K, R, SIG, T, is_put)
    assert v_in >= -1e-12 and v_out >= -1e-12
    assert abs(v_in + v_out - bs) <= 1e-12 * max(bs, 1.0)


@pytest.mark.parametrize("kind,is_put", CASES)
def test_far_barrier_out_is_vanilla_and_in_is_zero(kind, is_put):
    v = br.closed_form(kind, is_put, S0, 100.0, _H(kind, far=True), R, SIG, T)
    bs = br.black_scholes(S0, 100.0, R, SIG, T, is_put)
    if kind.endswith("-out"):
        assert abs(v - bs) <= 1e-12 * bs
    else:
        assert abs(v) <= 1e-12


@pytest.mark.parametrize("kind,is_put", CASES)
def test_bridge_monte_carlo_matches_the_closed_forms(kind, is_put):
    K = 100.0
    H = _H(kind)
    ref = br.closed_form(kind, is_put, S0, K, H, R, SIG, T)
    mc, se = br.bridge_mc(kind, is_put, S0, K, H, R, SIG, T, 200_000, 50, seed=11 + br.KINDS.index(kind))
    assert abs(mc - ref) <= 4 * se + 1e-12, (mc, se, ref)


def test_closed_form_refuses_a_knocked_spot():
    with pytest.raises(ValueError):
        br.closed_form("down-and-out", True, 80.0, 100.0, 85.0, R, SIG, T)
    with pytest.raises(ValueError):
        br.closed_form("up-and-in", False, 120.0, 100.0, 120.0, R, SIG, T)


@pytest.mark.parametrize("K,is_put", [(100.0, True), (100.0, False), (100.1, True), (100.1, False)])
def test_dead_spot_is_out_of_the_money_and_nearest(K, is_put):
    d = br.dead_spot(K, is_put)
    assert d.dtype == np.float32 and np.isfinite(d)
    pay = K - float(d) if is_put else float(d) - K
    assert pay <= 0.0
    # the next float32 towards the money would be in the money
    inner = np.nextafter(d, np.float32(-np.inf if is_put else np.inf))
    assert (K - float(inner) if is_put else float(inner) - K) > 0.0


@pytest.mark.parametrize("kind", br.KINDS)
def test_encoder_matches_a_per_path_loop(kind):
    rng = np.random.default_rng(3)
    N, M = 20, 300
    S = (100.0 * np.exp(np.cumsum(np.vstack([np.zeros((1, M)), 0.06 * rng.standard_normal((N, M))]), axis=0))).astype(
        np.float32)
    H = 90.0 if kind.startswith("down") else 110.0
    S[5, 0] = np.float32(H)  # exactly on the barrier: a hit
    K, is_put = 100.1, kind.startswith("up")
    enc = br.encode(S, kind, H, K=K, is_put=is_put)
    dead = br.dead_spot(K, is_put)
    ref = np.empty_like(S)
    for j in range(M):
        hit = False
        for t in range(N + 1):
            if t >= 1 and not hit:
                s = float(S[t, j])
                hit = s <= H if kind.startswith("down") else s >= H
            live = hit if kind.endswith("-in") else not hit
            ref[t, j] = S[t, j] if live else dead
    assert np.array_equal(enc, ref)
    hs = br.discrete_hit_steps(S, kind, H)
    assert hs[0] <= 5
    assert np.array_equal(br.encode(S, kind, H, hit_steps=hs, K=K, is_put=is_put), enc)


def test_bridge_probabilities_are_the_crossing_formula():
    rng = np.random.default_rng(5)
    N, P = 12, 64
    Z = rng.standard_normal((N, P)).astype(np.float32)
    H = 90.0
    p = br.bridge_probabilities(Z, S0, H, R, SIG, T)
    dt = T / N
    a = (R - 0.5 * SIG * SIG) * dt
    b = SIG * math.sqrt(dt)
    x = np.log(S0 / H) + np.cumsum(np.vstack([np.zeros((1, P)), a + b * Z.astype(np.float64)]), axis=0)
    want = np.exp(-2.0 * x[:-1] * x[1:] / (SIG * SIG * dt))
    assert np.allclose(p[:, :P], want, rtol=1e-4, atol=1e-6)


def test_compat_stub_without_arguments_keeps_the_reference_behaviour(capsys):
    from options_model_amd.compat import options_model_2 as v2
    out = v2.ExoticOptionPricer.price_barrier_option()
    assert isinstance(out, float) and math.isnan(out)
    assert capsys.readouterr().out == "Barrier option pricing not yet implemented.\n"


def test_facade_validates_before_touching_a_device():
    from options_model_amd import price_barrier_option
    kw = dict(S0=100.0, K=100.0, r=0.05, sigma=0.2, T=1.0, n_paths=1000, n_steps=10)
    with pytest.raises(ValueError):
        price_barrier_option(barrier=90.0, barrier_type="sideways-and-out", **kw)
    with pytest.raises(ValueError):
        price_barrier_option(barrier=90.0, style="bermudan", **kw)
    with pytest.raises(ValueError):
        price_barrier_option(barrier=90.0, monitoring="continuous", model="Heston", **kw)
    with pytest.raises(ValueError):
        price_barrier_option(barrier=float("nan"), **kw)
