"""The two choices the generators of full-storage matrices share (store_vec_width, omc_kernels.h): the pairs a thread owns
and the width of its stores.  Dividend, jump, multi-asset and barrier paths (DESIGN.md sections 11, 14, 15, 16).

  * the width hint (options "gbm_vec" / "heston_vec" = 1, 2, 4, 0) selects nothing but speed: the matrix kept through
    S_keep is the same, bit for bit.  A pair's operations depend neither on the pairs its thread owns besides it nor on
    its wave-mates; in the jump kernel a lane that does not jump executes the vanilla operations in both branches.
  * a leading dimension that only admits narrower stores (n_paths + 2: two floats, n_paths + 1: one) gives the columns
    of the aligned run, bit for bit, and leaves the padding columns alone; the pricing of that matrix has the aligned
    run's counts and its price to 1e-12 (the sweeps then sum in another order: same_pricing).  The barrier generator
    picks its pairs per thread from the geometry only, so its European sums are the aligned run's too.

The shape: 2,056 paths = 1,028 pairs, a multiple of 4 -- two workgroups at four pairs per thread, the second nearly
empty -- and 9 steps, which end inside a Philox block for GBM (4 steps per block) and Heston (2).
"""
import numpy as np
import pytest

from helpers.heston_qe_ref import SET_B
from options_model_amd import _ffi
from test_gpu_dividends import KEYS, at_steps, bits, params

pytestmark = pytest.mark.gpu

M, N = 2056, 9
SENTINEL = -7.0
JUMP = (4.0, -0.1, 0.15)
EURO = ("euro_out", "euro_out_se", "euro_in", "euro_in_se", "hit_prob")


def _params(model="gbm", scheme=0, **law):
    return params(model, scheme, M=M, N=N, seed=11, stream=5, pair_offset=321, **law)


def _dividends(ctx, p, keep, akeep):
    divs = at_steps(p, (1, 4, 5, N), [(0.9, "cash"), (0.015, "proportional"), (1.3, "cash"), (0.02, "proportional")])
    return ctx.price_american_div(p, 0.01, divs, S_keep=keep)


def _jumps(ctx, p, keep, akeep):
    return ctx.price_american_jump(p, JUMP, 0.01, S_keep=keep)


BASKET = _ffi.make_basket([100.0, 95.0], [0.2, 0.3], [0.01, 0.0], [0.6, 0.4], [[1.0, 0.5], [0.5, 1.0]], "basket")


def _basket(ctx, p, keep, akeep):
    return ctx.price_american_basket(p, BASKET, S_keep=keep, assets_keep=akeep)


def _barrier(ctx, p, keep, akeep):
    return ctx.price_barrier(p, "down-and-out", 80.0, monitoring="discrete", american=True, keep_paths=keep)


# name -> (the call, model, Heston scheme, the width option, asset matrices kept[, a Heston law of its own])
CASES = {"dividends-gbm": (_dividends, "gbm", 0, "gbm_vec", 0),
         "dividends-heston2": (_dividends, "heston", 2, "heston_vec", 0),
         "jumps-gbm": (_jumps, "gbm", 0, "gbm_vec", 0),
         "jumps-heston0": (_jumps, "heston", 0, "heston_vec", 0),
         "basket": (_basket, "gbm", 0, "gbm_vec", 2),
         "barrier": (_barrier, "gbm", 0, "gbm_vec", 0),
         # the QE scheme at the law whose waves mix its two branches (tests/helpers/heston_qe_ref.py, set B)
         "dividends-heston3": (_dividends, "heston", 3, "heston_vec", 0, SET_B),
         "jumps-heston3": (_jumps, "heston", 3, "heston_vec", 0, SET_B)}


def run(ctx, name, pad=0):
    """-> (result dict, the matrices as the call left them, padding columns included: [index or spot matrix, assets])"""
    call, model, scheme, _, d, *law = CASES[name]
    p = _params(model, scheme, **(law[0] if law else {}))
    keep = ctx.to_device(np.full((N + 1, M + pad), SENTINEL, np.float32))
    akeep = ctx.to_device(np.full((d, N + 1, M + pad), SENTINEL, np.float32)) if d else None
    try:
        out = call(ctx, p, keep, akeep)
        return out, [a.to_host() for a in (keep, akeep) if a is not None]
    finally:
        keep.free()
        if akeep is not None:
            akeep.free()


_aligned = {}


def aligned(ctx, name):
    """the run with leading dimension n_paths and the default width: computed once, shared, left unchanged"""
    if name not in _aligned:
        out, mats = run(ctx, name)
        for a in mats:
            assert np.isfinite(a).all() and (a != SENTINEL).all(), name  # every entry was written
            a.setflags(write=False)
        _aligned[name] = (out, mats)
    return _aligned[name]


def same_pricing(out, ref_out, what):
    """The sweeps on a matrix whose leading dimension is no multiple of 4 load single floats, and their float64 sums then
    run in another order (omc_lsm.hip, vec4_ok; tests/test_gpu_dividends.py checks the same): the same spots give the
    same decisions, hence identical counts; two orders of a float64 sum of n_paths non-negative terms differ by at most
    2 n_paths 2^-53 of it -- 4.6e-13 here, 1e-12 asked."""
    assert [out[k] for k in KEYS[5:]] == [ref_out[k] for k in KEYS[5:]], what
    assert out["price"] == pytest.approx(ref_out["price"], rel=1e-12, abs=0.0), what


@pytest.mark.parametrize("name", ["dividends-gbm", "dividends-heston2", "jumps-gbm", "jumps-heston0", "basket",
                                  "dividends-heston3", "jumps-heston3"])
def test_width_hint_selects_nothing_but_speed(ctx, name):
    ref_out, ref = aligned(ctx, name)
    option = CASES[name][3]
    try:
        for hint in (1, 2, 4, 0):
            ctx.set_option(option, hint)
            out, mats = run(ctx, name)
            for a, b in zip(mats, ref):
                assert np.array_equal(bits(a), bits(b)), (name, hint)
            assert [out[k] for k in KEYS] == [ref_out[k] for k in KEYS], (name, hint)
    finally:
        ctx.set_option(option, 0)


@pytest.mark.parametrize("pad", [2, 1])
@pytest.mark.parametrize("name", ["dividends-gbm", "jumps-gbm", "basket", "dividends-heston3", "jumps-heston3"])
def test_padded_leading_dimension_gives_the_aligned_columns(ctx, name, pad):
    ref_out, ref = aligned(ctx, name)
    out, mats = run(ctx, name, pad=pad)
    for a, b in zip(mats, ref):
        assert np.array_equal(bits(a[..., :M]), bits(b)), (name, pad)
        assert (a[..., M:] == SENTINEL).all(), (name, pad)
    same_pricing(out, ref_out, (name, pad))


def test_barrier_padded_leading_dimension_keeps_matrix_and_european_sums(ctx):
    ref_out, (ref,) = aligned(ctx, "barrier")
    out, (S,) = run(ctx, "barrier", pad=2)
    assert np.array_equal(bits(S[:, :M]), bits(ref))
    assert (S[:, M:] == SENTINEL).all()
    assert [out[k] for k in EURO] == [ref_out[k] for k in EURO]
    same_pricing(out, ref_out, "barrier")
    assert 0.0 < out["hit_prob"] < 1.0  # the barrier matters: some partners are knocked, some are not
