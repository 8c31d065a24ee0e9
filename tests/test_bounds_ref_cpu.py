"""CPU checks of the test helper behind the Andersen-Broadie bounds (tests/helpers/bounds_ref.py): the Bermudan lattice
against Black-Scholes and its own convergence, and the restated estimators on C-oracle paths."""
import math

import numpy as np
import pytest

from helpers import bounds_ref as br
from oracle import cpu as orc

S0, K, R, SIG, T = 100.0, 100.0, 0.05, 0.2, 1.0


def test_lattice_one_date_is_black_scholes():
    assert abs(br.lattice(S0, K, R, SIG, T, 1) - 5.573526) < 1e-5
    assert abs(br.lattice(S0, K, R, SIG, T, 1, is_put=False) - br.black_scholes(S0, K, R, SIG, T, False)) < 1e-9


def test_lattice_fifty_dates_and_monotone():
    vals = [br.lattice(S0, K, R, SIG, T, N) for N in (2, 10, 25, 50)]
    assert abs(vals[-1] - 6.079) < 2e-3, vals
    assert all(b > a for a, b in zip(vals, vals[1:])), vals
    # the call without dividends is never exercised early: the game is the European option (grid error ~1e-3)
    assert abs(br.lattice(S0, K, R, SIG, T, 50, is_put=False) - br.black_scholes(S0, K, R, SIG, T, False)) < 2e-3


def _textbook_policy(N, M=20000, stream=0):
    S = orc.gbm_paths(M, N, S0, R, SIG, T, 42, stream)
    d = orc.lsm_poly(S, K, R, T, True, "textbook")
    b = np.zeros((N + 1, 4))
    b[:, :3], b[:, 3] = d["betas"], d["nitm"]
    return b


def _restate(N, n_outer, n_inner, n_lower, betas4):
    Sl = orc.gbm_paths(n_lower, N, S0, R, SIG, T, 42, 1)
    lo = br.lower_bound(Sl, K, R, T, True, betas4)
    So = orc.gbm_paths(n_outer, N, S0, R, SIG, T, 42, 2)
    Z = orc.gbm_normals(n_outer * (N + 1) * n_inner // 2, N, 42, 3)
    inner = br.inner_from_normals(Z, So, n_inner, lambda z, s0: orc.gbm_paths_from_normals(z, s0, R, SIG, T))
    up = br.upper_bound(So, inner, K, R, T, True, betas4)
    return lo, up


def test_restated_upper_above_lower():
    N = 8
    lo, up = _restate(N, 64, 256, 20000, _textbook_policy(N))
    assert lo["ties"] == 0 and up["ties"] == 0
    assert up["upper"] >= lo["lower"], (lo, up)
    V = br.lattice(S0, K, R, SIG, T, N)
    assert lo["lower"] - 4 * lo["se_lower"] <= V <= up["upper"] + 4 * up["se_upper"], (lo, up, V)
    assert up["inner_path_steps"] > 0


def test_restated_one_date_samples_are_q0():
    lo, up = _restate(1, 32, 64, 4000, np.zeros((2, 4)))
    np.testing.assert_allclose(up["samples"], up["q"][:, 0], rtol=1e-14, atol=1e-13)  # Z_1 - (Z_1 - Q^_0), rounded
    assert up["upper"] == pytest.approx(up["q"][:, 0].mean(), rel=1e-14)
    assert lo["n_exercised"] == 0
    assert up["inner_path_steps"] == 32 * 64


def test_tightness_threshold_from_restatement():
    """The duality gap of the textbook policy at N = 50 on a CPU-sized run: the GPU bracket test asserts upper - lower
    < 0.02 V for the put; the restatement shows where that threshold stands against the gap itself."""
    N = 50
    lo, up = _restate(N, 64, 128, 20000, _textbook_policy(N))
    V = br.lattice(S0, K, R, SIG, T, N)
    gap = up["upper"] - lo["lower"]
    se = math.hypot(lo["se_lower"], up["se_upper"])
    assert gap - 3 * se < 0.02 * V, (gap, se, V)
