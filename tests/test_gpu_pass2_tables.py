"""Pass 2 on per-step exercise tables (option "pass2_tables", default 1; options_model_amd/csrc/omc_crit.h) against the
float64 decisions it replaces (option value 0): the same decisions, so every result field is bit-equal.

Covered: put and call, S0 != K, sigma up to 0.8, N in {2, 3, 50, 252}, folded storage with column counts that run each of
the VEC 1 / 2 / 4 sweeps, single calls and the sequence call; steps forced onto the float64 fallback inside the table
sweep; and on the device, every non-negative float32 spot of every step against the float64 decision
(omc_pass2_tables_check) for the headline fits and fuzzed ones."""
import numpy as np
import pytest

from options_model_amd import _ffi

pytestmark = pytest.mark.gpu

KEYS = ("price", "sum", "sumsq", "n_exercised", "n_zero", "sum_nitm", "folded")


@pytest.fixture
def tctx(ctx):
    ctx.set_option("fold_antithetic", 2)
    yield ctx
    ctx.set_option("fold_antithetic", 1)
    ctx.set_option("pass2_tables", 1)


def _both(ctx, p):
    out = {}
    for v in (0, 1):
        ctx.set_option("pass2_tables", v)
        out[v] = ctx.price_american(p)
    ctx.set_option("pass2_tables", 1)
    return out[0], out[1]


CASES = [
    # (is_put, S0, K, sigma, N, paths, seed)
    (True, 100.0, 100.0, 0.2, 252, 200_000, 1),
    (False, 100.0, 100.0, 0.2, 252, 200_000, 2),
    (True, 90.0, 100.0, 0.8, 50, 100_002, 3),    # odd column count: the VEC 1 sweep
    (False, 110.0, 100.0, 0.8, 50, 100_006, 4),  # (M / 2) % 4 == 3
    (True, 120.0, 100.0, 0.5, 3, 65_536, 5),
    (False, 80.0, 100.0, 0.05, 2, 65_536, 6),
    (True, 100.0, 95.0, 0.3, 50, 131_080, 7),
    (False, 100.0, 105.0, 0.6, 3, 4_000, 8),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{'put' if c[0] else 'call'}-S{c[1]:g}-K{c[2]:g}-s{c[3]:g}-N{c[4]}-M{c[5]}"
                                             for c in CASES])
def test_tables_bit_equal_to_float64_decisions(tctx, case):
    is_put, S0, K, sigma, N, M, seed = case
    p = _ffi.make_params(semantics="two_pass", is_put=is_put, S0=S0, K=K, sigma=sigma, n_paths=M, n_steps=N, seed=seed,
                         stream=seed)
    a, b = _both(tctx, p)
    assert a["folded"] == 1
    assert [a[k] for k in KEYS] == [b[k] for k in KEYS], (a, b)
    assert b["n_exercised"] > 0 or N == 2


def test_vec4_sweep_bit_equal(tctx):
    """2^21 stored columns and more: the 16-byte (VEC 4) sweep"""
    p = _ffi.make_params(semantics="two_pass", is_put=True, n_paths=1 << 22, n_steps=9, sigma=0.4, seed=9, stream=1)
    a, b = _both(tctx, p)
    assert [a[k] for k in KEYS] == [b[k] for k in KEYS], (a, b)


def test_sequence_and_batch_bit_equal(tctx):
    ps = [_ffi.make_params(semantics="two_pass", is_put=bool(i & 1), S0=95.0 + 5 * i, sigma=0.2 + 0.1 * i, n_paths=70_000,
                           n_steps=40, seed=3, stream=i) for i in range(3)]
    out = {}
    for v in (0, 1):
        tctx.set_option("pass2_tables", v)
        out[v] = tctx.price_american_seq(ps)
    for a, b in zip(out[0], out[1]):
        assert [a[k] for k in KEYS] == [b[k] for k in KEYS], (a, b)


def _fold_cK(p):
    from oracle import cpu as orc
    c0, g = orc.fold_constants(p.S0, p.K, p.r, p.sigma, p.T, p.n_steps)
    return orc.fold_table(p.n_steps, c0, g)


@pytest.mark.parametrize("is_put", [True, False], ids=["put", "call"])
def test_exhaustive_headline_fits(ctx, is_put):
    """the headline pricing's fits (1M paths x 252 steps): the table decision equals the float64 decision at every
    non-negative float32 spot, every step, both partners -- on the device, with the sweep's own expressions"""
    p = _ffi.make_params(semantics="two_pass", is_put=is_put, n_paths=1_000_000, n_steps=252, seed=42, stream=0)
    betas = ctx.price_american_greeks(p, want_betas=True)["betas"]
    mism, irr = ctx.pass2_tables_check(is_put, p.K, betas, _fold_cK(p))
    assert int(mism.sum()) == 0, np.argwhere(mism)
    assert int(irr.sum()) == 0


def test_exhaustive_fuzz_fits(ctx):
    """random fits, both signs of b2, b2 = 0, no-fit steps; and one run with every third step forced irregular"""
    rng = np.random.default_rng(17)
    N = 24
    for case in range(6):
        is_put = bool(case & 1)
        betas = np.zeros((N + 1, 4))
        betas[:, 0] = rng.normal(2.0, 3.0, N + 1)
        betas[:, 1] = rng.normal(-50.0, 60.0, N + 1)
        betas[:, 2] = rng.normal(0.0, 300.0, N + 1) * (rng.random(N + 1) < 0.7)
        betas[:, 3] = np.where(rng.random(N + 1) < 0.9, 1000.0, 0.0)  # n <= 0.5: no fit at that step
        cK = 100.0 * np.exp(rng.normal(0.0, 0.3)) * np.cumprod(np.full(N + 1, 1.0 + rng.normal(0, 0.01)))
        mism, irr = ctx.pass2_tables_check(is_put, rng.uniform(80, 120), betas, cK, irregular_every=3 if case == 5 else 0)
        assert int(mism.sum()) == 0, (case, np.argwhere(mism))
        if case == 5:
            assert all(irr[t] for t in range(3, N, 3))


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("M", [100_002, 200_000, 1 << 22], ids=["vec1", "vec2", "vec4"])
def test_forced_irregular_steps_bit_equal(tctx, every, M):
    """steps marked irregular are decided inside the table sweep by its float64 fallback: still bit-equal"""
    p = _ffi.make_params(semantics="two_pass", is_put=bool(M & 2), n_paths=M, n_steps=50 if M < (1 << 22) else 9,
                         sigma=0.4, seed=5, stream=M % 7)
    tctx.set_option("pass2_tables", 0)
    a = tctx.price_american(p)
    tctx.set_option("pass2_tables", 1)
    tctx.set_option("pass2_tables_irregular_every", every)
    try:
        b = tctx.price_american(p)
    finally:
        tctx.set_option("pass2_tables_irregular_every", 0)
    assert [a[k] for k in KEYS] == [b[k] for k in KEYS], (a, b)
