"""tests/helpers/european_ref.py pinned without a GPU: the restatement against an independent exact evaluation of the
documented formulas (fractions.Fraction), known answers, the two bounds biting on the mutations they are there for at every
shape of tests/test_gpu_european_sums.py, and that file's shape lists holding every layout of the kernels -- derived from
the kernels' constants (kBlock 256, kMaxLsmBlocks 1024, kPayChunk 4096, the barrier_vec rule), not from a list of names."""
import math
from fractions import Fraction

import numpy as np
import pytest

import test_gpu_european_sums as gs
from helpers import european_ref as er
from oracle import cpu as orc

S0, K, R, SIG, T = 100.0, 100.0, 0.05, 0.2, 1.0
DF = math.exp(-R * T)


def _exact(ST, k, df, is_put, discount_terms):
    """the documented formula, term by term in rationals: the sums exact, then rounded once"""
    tot, tot2, n_zero = Fraction(0), Fraction(0), 0
    for s in np.asarray(ST, np.float32):
        p = Fraction(k) - Fraction(float(s)) if is_put else Fraction(float(s)) - Fraction(k)
        p = Fraction(float(p)) if p > 0 else Fraction(0)            # K - (double)s is ONE float64 operation
        if discount_terms and p > 0:
            p = Fraction(float(p * Fraction(df)))                   # so is p * df
        n_zero += p == 0
        tot += p
        tot2 += Fraction(float(p * p))                              # and the square
    return tot, tot2, n_zero


@pytest.fixture(scope="module")
def spots():
    S = orc.gbm_paths(4096, 10, S0, R, SIG, T, 42, 3)
    S.setflags(write=False)
    return S[-1]


@pytest.mark.parametrize("discount_terms", [True, False])
@pytest.mark.parametrize("is_put", [True, False])
def test_sums_are_the_exact_sums_rounded_once(spots, is_put, discount_terms):
    got = er.sums(spots, K, DF, is_put, discount_terms)
    tot, tot2, n_zero = _exact(spots, K, DF, is_put, discount_terms)
    assert (got["sum"], got["sumsq"]) == (float(tot), float(tot2))  # to the last bit
    assert (got["n_zero"], got["n_paths"], got["sum_abs"]) == (n_zero, 4096, got["sum"])
    assert 0 < n_zero < 4096
    mean, se = er.mean_se(got["sum"], got["sumsq"], 4096)
    m = Fraction(got["sum"]) / 4096
    var = Fraction(got["sumsq"]) / 4096 - m * m
    assert mean == float(m)
    assert se == pytest.approx(math.sqrt(var / 4096), rel=1e-12)
    # the strike kernels' host-side discounting is the per-term discounting up to the roundings of the terms
    if discount_terms:
        raw = er.sums(spots, K, DF, is_put, False)
        assert raw["sum"] * DF == pytest.approx(got["sum"], rel=1e-14) and raw["n_zero"] == got["n_zero"]


def test_known_answers():
    # M = 2, one zero payoff: put on (90, 110) at K = 100, df = 0.5 -> terms (5, 0)
    s = er.sums(np.float32([90.0, 110.0]), 100.0, 0.5, True, True)
    assert (s["sum"], s["sumsq"], s["n_zero"], s["sum_abs"], s["n_paths"]) == (5.0, 25.0, 1, 5.0, 2)
    mean, se = er.mean_se(s["sum"], s["sumsq"], 2)
    assert mean == 2.5 and se == math.sqrt((12.5 - 6.25) / 2)
    # the raw payoffs of the strike kernels
    s = er.sums(np.float32([90.0, 110.0]), 100.0, 0.5, True, False)
    assert (s["sum"], s["sumsq"]) == (10.0, 100.0)
    # all-zero payoffs: se exactly 0
    s = er.sums(np.float32([101.0, 110.0, 250.0]), 100.0, DF, True, True)
    assert (s["sum"], s["sumsq"], s["n_zero"]) == (0.0, 0.0, 3)
    assert er.mean_se(0.0, 0.0, 3) == (0.0, 0.0)
    # equal payoffs: the variance cancels to 0 (or below) and is clamped
    assert er.mean_se(3 * 0.1, 3 * 0.1 * 0.1, 3)[1] < 1e-9
    # a strike equal to a spot's exact float32 value: payoff exactly 0, counted in n_zero, for both sides
    spot = np.float32(100.1)
    assert float(spot) != 100.1
    for is_put in (True, False):
        s = er.sums(np.float32([spot, 90.0, 120.0]), float(spot), DF, is_put, True)
        assert s["n_zero"] == 2 and s["sum"] > 0.0
        assert er.sums(np.float32([spot]), 100.1, DF, is_put, True)["n_zero"] == (0 if is_put else 1)  # the double is not the float


def test_barrier_sums_split_the_vanilla_by_the_hit_flag(spots):
    rng = np.random.default_rng(1)
    hit = rng.random(spots.size) < 0.3
    b = er.barrier_sums(spots, hit, K, DF, False)
    van = er.sums(spots, K, DF, False, True)
    assert b["out"]["sum"] + b["in"]["sum"] == pytest.approx(van["sum"], rel=1e-15)
    assert b["out"]["sumsq"] + b["in"]["sumsq"] == pytest.approx(van["sumsq"], rel=1e-15)
    assert b["out"]["sum"] == er.sums(spots[~hit], K, DF, False, True)["sum"]
    assert b["in"]["sumsq"] == er.sums(spots[hit], K, DF, False, True)["sumsq"]
    assert (b["n_hit"], b["hit_prob"]) == (int(hit.sum()), hit.sum() / spots.size)
    assert (b["euro_out"], b["euro_out_se"]) == er.mean_se(b["out"]["sum"], b["out"]["sumsq"], spots.size)
    assert (b["euro_in"], b["euro_in_se"]) == er.mean_se(b["in"]["sum"], b["in"]["sumsq"], spots.size)
    none = er.barrier_sums(spots, np.zeros(spots.size, bool), K, DF, False)
    assert (none["euro_in"], none["euro_in_se"], none["hit_prob"]) == (0.0, 0.0, 0.0) and none["euro_out"] == van["sum"] / 4096
    every = er.barrier_sums(spots, np.ones(spots.size, bool), K, DF, False)
    assert (every["euro_out"], every["euro_out_se"], every["hit_prob"]) == (0.0, 0.0, 1.0)


# ------------------------------------------------------------------ the bounds bite
LARGEST = max(gs.EURO_BIG[0], gs.EURO_BIG_SINGLE[0], gs.BARRIER_BIG[0], max(gs.STRIKE_M), gs.SURFACE_M)


def _rejects(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


@pytest.mark.parametrize("M", [2, 4098, LARGEST])
def test_bounds_reject_a_lost_term_an_m_minus_1_and_a_doubled_square(M):
    assert LARGEST == 524_802
    ST = orc.gbm_paths(M, 3, S0, R, SIG, T, 42, 9)[-1]
    # M = 2: a put deep in the money, so that both partners pay; else at the money, on the side where the first term pays
    k = K if M > 2 else 150.0
    is_put = bool(er.terms(ST[:1], k, DF, True, True)[0] > 0.0)
    p = er.terms(ST, k, DF, is_put, True)
    ref = er.sums(ST, k, DF, is_put, True)
    assert p[0] > 0.0 and p.min() >= 0.0 and (M > 2 or p.min() > 0.0)
    mean, se = er.mean_se(ref["sum"], ref["sumsq"], M)
    # the restatement itself, and a float64 sum in another order, pass
    er.sums_close(ref["sum"], ref["sum"], ref["sum_abs"], M)
    er.sums_close(float(np.sum(p[::-1])), ref["sum"], ref["sum_abs"], M)
    er.sums_close(float(np.sum((p * p).reshape(2, -1).sum(axis=0))), ref["sumsq"], ref["sumsq"], M)
    er.sums_close(Fraction(mean) * M, ref["sum"], ref["sum_abs"], M)
    er.se_close(se, ref["sum"], ref["sumsq"], M)
    er.se_close(se * DF, ref["sum"], ref["sumsq"], M, scale=DF)
    er.se_close(se * math.sqrt(M), ref["sum"], ref["sumsq"], M, scale=np.sqrt(np.longdouble(M)))
    # one term removed: near the front, the end of the first half and the end, the nearest term there that is an ordinary
    # one (a tenth of the mean or more: a lost term of 1e-9 is lost to any bound that admits another summation order)
    big = np.nonzero(p >= 0.1 * mean)[0]
    for j in {int(big[0]), int(big[big < max(M // 2, 1)][-1]), int(big[-1])}:
        _rejects(er.sums_close, math.fsum(np.delete(p, j)), ref["sum"], ref["sum_abs"], M)
        _rejects(er.sums_close, math.fsum(np.delete(p * p, j)), ref["sumsq"], ref["sumsq"], M)
        lost = er.mean_se(math.fsum(np.delete(p, j)), ref["sumsq"], M)[1]
        _rejects(er.se_close, lost, ref["sum"], ref["sumsq"], M)
    # an M - 1 divisor of the variance
    var = ref["sumsq"] / M - mean * mean
    assert var > 0.0
    _rejects(er.se_close, math.sqrt(var / (M - 1)), ref["sum"], ref["sumsq"], M)
    _rejects(er.se_close, DF * math.sqrt(var / (M - 1)), ref["sum"], ref["sumsq"], M, scale=DF)
    _rejects(er.se_close, math.sqrt(var * M / (M - 1)), ref["sum"], ref["sumsq"], M, scale=np.sqrt(np.longdouble(M)))
    # a doubled square, a square added once per pair, a discount factor applied once to a squared sum
    q = p * p
    _rejects(er.sums_close, math.fsum(q) + float(q[0]), ref["sumsq"], ref["sumsq"], M)
    _rejects(er.se_close, er.mean_se(ref["sum"], math.fsum(q) + float(q[0]), M)[1], ref["sum"], ref["sumsq"], M)
    _rejects(er.sums_close, math.fsum(q[:M // 2]), ref["sumsq"], ref["sumsq"], M)
    raw = er.sums(ST, k, DF, is_put, False)
    _rejects(er.se_close, er.mean_se(DF * raw["sum"], DF * raw["sumsq"], M)[1], ref["sum"], ref["sumsq"], M)
    # se of all-zero terms must be exactly 0
    er.se_close(0.0, 0.0, 0.0, M)
    _rejects(er.se_close, 5e-324, 0.0, 0.0, M)


# ------------------------------------------------------------------ the shape lists hold every layout
B, MAXB, CHUNK, WAVE = (er.LAYOUT[k] for k in ("block", "max_blocks", "pay_chunk", "wave"))


def test_layout_constants_are_the_kernels():
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "options_model_amd", "csrc")
    text = {f: open(os.path.join(src, f)).read() for f in ("omc_kernels.h", "omc_paths.hip", "omc_barrier.hip", "omc_device.h")}
    assert int(re.search(r"constexpr int kMaxLsmBlocks = (\d+);", text["omc_kernels.h"]).group(1)) == MAXB
    assert int(re.search(r"constexpr int kPayChunk = (\d+);", text["omc_paths.hip"]).group(1)) == CHUNK
    blocks = [re.search(r"constexpr int kBlock = (\d+);", t) for t in text.values()]
    assert [int(m.group(1)) for m in blocks if m] == [B]
    assert "((a.paths.n_paths / 2) % 4) == 0 ? 4 : 1" in text["omc_barrier.hip"]


@pytest.mark.parametrize("anti", [True, False])
def test_european_shapes_hold_every_layout_of_terminal_body(anti):
    Ms = gs.EURO_M if anti else gs.EURO_M_SINGLE
    big, big_n = gs.EURO_BIG if anti else gs.EURO_BIG_SINGLE
    lay = [er.terminal_layout(M, anti) for M in Ms]
    assert any(P == (1 if anti else 2) for P, *_ in lay)                                   # the fewest work items
    assert any(nb == 1 and P < B and P % WAVE for P, nb, _, _ in lay)                      # one workgroup, a wave not full
    assert any(nb == 1 and P == B for P, nb, _, _ in lay)                                  # exactly one workgroup
    assert any(nb == 2 and last < WAVE for _, nb, _, last in lay)                          # a second, nearly empty one
    assert any(nb > 2 and last < B for _, nb, _, last in lay)                              # many, the last ragged
    assert all(second == 0 for *_, second, _ in lay)
    P, nb, second, _ = er.terminal_layout(big, anti)
    assert nb == MAXB and 0 < second <= B + 1 and second % B                               # a second trip for a few lanes
    if not anti:
        assert any(M % 2 for M in Ms) and big % 2                                          # odd path counts
    assert all(M % 2 == 0 for M in Ms) or not anti
    # every N of the list ends on (N % steps == 0) and inside a Philox block: 4 steps per block for GBM, 2 for Heston
    for steps in (4, 2):
        assert {n % steps == 0 for n in gs.EURO_N} == {True, False}
    assert 1 in gs.EURO_N and max(gs.EURO_N) > 8 and big_n % 4 and big_n % 2


def test_barrier_shapes_hold_every_layout_of_the_barrier_body():
    lay = {M: er.barrier_layout(M) for M in gs.BARRIER_M}
    assert any(M == 2 and v == 1 for M, (v, *_) in lay.items())                            # one pair, VEC 1
    assert any(v == 4 and nb == 1 and th == 1 for v, nb, th, _ in lay.values())            # VEC 4 in one thread
    assert any(v == 1 and nb >= 3 and th < WAVE for v, nb, th, _ in lay.values())          # VEC 1, several workgroups
    assert any(v == 4 and nb == 1 and th == B for v, nb, th, _ in lay.values())            # exactly one VEC-4 workgroup
    assert any(v == 4 and nb == 2 and th < WAVE for v, nb, th, _ in lay.values())          # a second, nearly empty one
    assert all(trips == 1 for *_, trips in lay.values())
    v, nb, th, trips = er.barrier_layout(gs.BARRIER_BIG[0])
    assert v == 1 and nb == B + 1 and trips == 2                                           # the finalize's second trip: one thread
    assert all(M % 2 == 0 for M in gs.BARRIER_M + [gs.BARRIER_BIG[0]])
    for steps in (4, 2):                                                                   # on and inside a Philox block
        assert {n % steps == 0 for n in gs.BARRIER_N + [8]} == {True, False}
    assert any(n % 4 and n % 2 for n in gs.BARRIER_N)
    kinds = {(m[1], m[2], m[3]) for m in gs.BARRIER_MODELS}
    assert kinds == {("gbm", 0, "discrete"), ("gbm", 0, "continuous")} | {("heston", s, "discrete") for s in (0, 1, 2)}


def test_strike_shapes_hold_every_layout_of_the_chunked_reduction():
    lay = [er.strikes_layout(M) for M in gs.STRIKE_M]
    assert any(n == 1 and last == 2 for n, last in lay)                                    # one pair
    assert any(n == 1 and 2 < last < B for n, last in lay)                                 # below one block
    assert any(n == 1 and last == CHUNK for n, last in lay)                                # exactly one chunk
    assert any(n == 2 and last == 2 for n, last in lay)                                    # a chunk of two spots
    assert any(n == 2 and B < last < CHUNK and last % B for n, last in lay)                # two chunks, the second ragged
    assert any(n >= 4 and last == 2 for n, last in lay)                                    # four chunks, the last of two spots
    assert all(M % 2 == 0 for M in gs.STRIKE_M)
    assert set(gs.STRIKE_COUNTS) == {1, 3, 61} and {n % 2 for n in gs.STRIKE_N} == {0, 1} and 1 in gs.STRIKE_N
    n, last = er.strikes_layout(gs.SURFACE_M)
    assert n == 2 and last == 2 and (gs.SURFACE_M + 63) // 64 * 64 > gs.SURFACE_M          # the row stride is not M
