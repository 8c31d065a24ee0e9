"""CPU checks of the Greeks and bounds sweeps of tests/test_gpu_fuzz.py (13 and 14): their case generators deal every kernel
variant and code path they are there for, whatever the seed; every default-seed case runs through the numpy restatements
(tests/helpers/greeks_ref.py, bounds_ref.py) on C-oracle paths without a single tie (a decision within 1e-10 K of the
continuation value: the one thing that excuses a case from its value comparison on the device); and bounds_ref.q_rows on
sampled outer paths is upper_bound's Q^ on those paths."""
import numpy as np
import pytest

import test_gpu_fuzz as fz
from helpers import bounds_ref as br
from helpers import greeks_ref as gr
from oracle import cpu as orc

GREEKS = fz._greeks_cases(16, 131313)
BOUNDS = fz._bounds_cases(12, 141414)
VARIANTS = ((1, True), (2, True), (1, False), (2, False))


@pytest.mark.parametrize("seed", [131313, 0, 1, 2, 3, 20250101, 2 ** 31 - 1])
@pytest.mark.parametrize("n", [16, 80])
def test_greeks_generator_deals_every_kernel_variant(seed, n):
    cases = fz._greeks_cases(n, seed)
    assert len(cases) == n
    for v in VARIANTS:
        both = {c["given"] for c in cases[:8] if fz._greeks_variant(c) == v}
        assert sum(fz._greeks_variant(c) == v for c in cases) >= 2 and both == {False, True}, (seed, v)
    # what the fixed shapes of tests/test_gpu_greeks.py leave out: no sweep at all, one row, walk_rows' batches of 8
    assert {c["N"] for c in cases[:12]} == {1, 2, 3, 7, 8, 9, 15, 16, 17, 33, 50, 70}
    for c in cases:
        assert c["M"] % 2 == 0 or not c["antithetic"]  # the library refuses odd antithetic path counts (-3)
        assert not c["fold"] or (c["model"] == "gbm" and c["antithetic"])


def test_greeks_default_draw_has_the_other_edges():
    assert {c["off"] for c in GREEKS} == {0, 12345, 2 ** 33 + 7} and len({c["bump"] for c in GREEKS}) >= 3
    assert any(c["r"] == 0.0 for c in GREEKS) and any(c["T"] != 1.0 for c in GREEKS)
    assert any(c["model"] == "heston" for c in GREEKS)


@pytest.mark.parametrize("seed", [141414, 0, 1, 2, 3, 20250101, 2 ** 31 - 1])
@pytest.mark.parametrize("n", [12, 60])
def test_bounds_generator_deals_every_code_path(seed, n):
    cases = fz._bounds_cases(n, seed)
    assert len(cases) == n
    assert 2 * sum(fz._bounds_refills(c) for c in cases) >= n
    assert sum(fz._bounds_second_item(c) and c["n_inner"] <= 130 for c in cases) >= 2 * (n // 12)
    assert sum(fz._bounds_lower_strides(c) for c in cases) >= 2 * (n // 12)
    assert sum(c["n_inner"] == 2 for c in cases) >= n // 12 and sum(c["policy"] == "given" for c in cases) >= n // 12
    assert {c["N"] for c in cases[:12]} == {1, 2, 3, 5, 7, 9, 13, 17}
    for c in cases:  # inside the library's caps (-16) and the restatement's budget; q's tolerance needs n_inner <= 2048
        assert c["n_outer"] * (c["N"] + 1) * c["n_inner"] <= 2 ** 32 and c["n_inner"] <= 2048
        assert c["n_outer"] * c["N"] * c["n_inner"] <= fz._BOUNDS_BUDGET
        assert c["n_lower"] % 2 == c["n_outer"] % 2 == c["n_inner"] % 2 == 0


def _greeks_restated(c):
    """the restatement of a Greeks case on C-oracle paths, the policy fitted by the oracle's two-pass flow"""
    N, h = c["N"], fz._GREEKS_HESTON
    cK = None
    if c["fold"]:
        c0, g = orc.fold_constants(c["S0"], c["K"], c["r"], c["sigma"], c["T"], N)
        cK = orc.fold_table(N, c0, g)

    def paths(stream):
        if c["model"] == "heston":
            return orc.heston_paths(c["M"], N, c["S0"], c["r"], c["T"], h["v0"], h["kappa"], h["theta"], h["xi"], h["rho"],
                                    c["seed"], stream, c["off"], c["scheme"])
        if c["fold"]:
            return orc.gbm_paths(c["M"] // 2, N, c["S0"], c["r"], c["sigma"], c["T"], c["seed"], stream, c["off"], 0)
        return orc.gbm_paths(c["M"], N, c["S0"], c["r"], c["sigma"], c["T"], c["seed"], stream, c["off"], int(c["antithetic"]))

    def fit(S):
        if c["fold"]:
            ref = orc.lsm_two_pass_folded(S, c["K"], c["r"], c["T"], c["is_put"], c0, g)
        else:
            ref = orc.lsm_poly(S, c["K"], c["r"], c["T"], c["is_put"], "two_pass")
        return gr.betas4_from(ref["betas"], ref["nitm"]), ref

    S = paths(c["stream"])
    assert S.shape[1] == fz._greeks_cols(c)
    b4, ref = fit(S)
    if c["given"]:
        b4 = fz._holes(fit(paths(c["stream"] + 7))[0], c["holes"])
        ref = None
    g_ = gr.greeks(S, c["K"], c["r"], c["T"], c["is_put"], b4, c["S0"], c["sigma"], h=c["bump"], cK=cK, gbm=(c["model"] == "gbm"))
    return g_, ref


@pytest.mark.parametrize("case", GREEKS, ids=fz._greeks_id)
def test_greeks_case_restates_without_ties(case):
    g, ref = _greeks_restated(case)
    assert g["ties"] == [0, 0, 0], g["ties"]
    assert g["n_paths"] == case["M"]
    if ref is not None:  # the fitted policy: the base scenario is the oracle's two-pass pricing
        assert g["n_exercised"] == ref["n_exercised"] and g["n_zero"] == ref["n_zero"]
        assert abs(g["price"] - ref["price"]) <= 1e-12 * abs(ref["price"])
    assert np.isfinite([g[k] for k in ("price", "delta", "gamma", "price_up", "price_down")]).all()


def _bounds_restated(c):
    N, K, r, T = c["N"], c["K"], fz._BOUNDS_R, fz._BOUNDS_T

    def fits(policy, stream):
        f = orc.lsm_poly(orc.gbm_paths(c["M"], N, c["S0"], r, c["sigma"], T, c["seed"], stream), K, r, T, c["is_put"], policy)
        return gr.betas4_from(f["betas"], f["nitm"])

    b4 = fz._holes(fits("textbook", c["stream"] + 9), c["holes"]) if c["policy"] == "given" else fits(c["policy"], c["stream"])
    Sl = orc.gbm_paths(c["n_lower"], N, c["S0"], r, c["sigma"], T, c["seed"], c["stream"] + 1)
    So = orc.gbm_paths(c["n_outer"], N, c["S0"], r, c["sigma"], T, c["seed"], c["stream"] + 2)
    inner = br.inner_by_item(lambda off, n: orc.gbm_normals(n, N, c["seed"], c["stream"] + 3, off), So, c["n_inner"],
                             lambda z, s0: orc.gbm_paths_from_normals(z, s0, r, c["sigma"], T))
    lo = br.lower_bound(Sl, K, r, T, c["is_put"], b4)
    up = br.upper_bound(So, inner, K, r, T, c["is_put"], b4)
    return b4, So, inner, lo, up


@pytest.mark.parametrize("case", BOUNDS, ids=fz._bounds_id)
def test_bounds_case_restates_without_ties(case):
    c = case
    N, K, r, T = c["N"], c["K"], fz._BOUNDS_R, fz._BOUNDS_T
    b4, So, inner, lo, up = _bounds_restated(c)
    assert lo["ties"] == 0 and up["ties"] == 0
    assert up["q"].shape == (c["n_outer"], N) and np.all(up["q"] >= 0.0)
    assert c["n_outer"] * c["n_inner"] * N <= up["inner_path_steps"] <= c["n_outer"] * c["n_inner"] * N * (N + 1) // 2
    assert lo["se_cancel"] >= 1.0 and up["se_cancel"] >= 1.0
    # q_rows on sampled outer paths (first, last, a partner column) is upper_bound's Q^ there, and so is the walk
    rows = sorted({0, c["n_outer"] // 2, c["n_outer"] - 1})
    qr = br.q_rows(So, inner, rows, K, r, T, c["is_put"], b4)
    np.testing.assert_array_equal(qr["q"], up["q"][rows])
    wk = br.walk_rows(So, qr["q"], rows, K, r, T, c["is_put"], b4)
    np.testing.assert_array_equal(wk["samples"], up["samples"][rows])
    assert wk["zmax"] <= up["zmax"]


def test_normals_by_item_are_the_whole_call_normals():
    """inner_by_item (every item's normals at its own pair offset) builds the spots of inner_from_normals (one array over
    the whole call), bit for bit -- the layout DESIGN.md 12.1 documents."""
    N, n_outer, n_inner, r, sig, T = 5, 6, 130, 0.05, 0.2, 1.0
    So = orc.gbm_paths(n_outer, N, 100.0, r, sig, T, 42, 2)
    spots = lambda z, s0: orc.gbm_paths_from_normals(z, s0, r, sig, T)  # noqa: E731
    a = br.inner_from_normals(orc.gbm_normals(n_outer * (N + 1) * n_inner // 2, N, 42, 3), So, n_inner, spots)
    b = br.inner_by_item(lambda off, n: orc.gbm_normals(n, N, 42, 3, off), So, n_inner, spots)
    for i in range(n_outer):
        for t in range(N):
            np.testing.assert_array_equal(a(i, t), b(i, t))
