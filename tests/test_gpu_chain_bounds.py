"""omc_price_american_chain_bounds against every entry's own single call on the device (the contract
of include/omc_chain_bounds.h): omc_price_american_bounds under GBM, omc_price_american_bounds_heston under Heston, same sizes,
seed and streams, both run in the same test on the same context.

  exact at any sizes      betas, lower, se_lower, n_exercised_lower, inner_path_steps: equal bit for bit
  n_inner <= 128          q, samples, upper, se_upper too: no lane is refilled, the wave sum has one order
  n_inner > 128           q and upper differ by the order of float64 sums of non-negative terms.  Measured on an MI355X over
                          helpers/chain_bounds_catalogue.TOLERANCE_CASES and the refilling ones of 200 seeded fuzz cases (87
                          cases), each entry against its own single call: the worst relative deviation of `upper` 2.997e-16
                          and of q against max|q| 2.920e-16 (MEASURED_UPPER_REL / MEASURED_Q_REL = 3.0e-16 in
                          helpers/chain_bounds_case.py); the tests assert 4x those, 1.2e-15, which must stay below the 1e-9
                          of the README's price contract.
  a chain of one entry    satisfies all of it; two identical entries give identical outputs
  simulated steps         at least the largest of the entries' inner_path_steps, at most their sum, the entry's own when all
                          entries of a group are the same
"""
import numpy as np
import pytest

from helpers import chain_bounds_case as cc
from helpers import chain_bounds_catalogue as cat

pytestmark = pytest.mark.gpu

UPPER_REL = 4.0 * cc.MEASURED_UPPER_REL
Q_REL = 4.0 * cc.MEASURED_Q_REL


def _against_single_calls(ctx, case):
    outs, info = cc.run_chain(ctx, case)
    assert len(outs) == len(case["strikes"])
    for e, got in enumerate(outs):
        cc.compare(case, got, cc.run_single(ctx, case, e), UPPER_REL, Q_REL)
    cc.check_steps(outs, info)
    assert info["entries_per_group"] == cc.CAP  # (16 (N+1) bytes of tables per entry: far below the LDS rule's 65536)
    return outs, info


@pytest.mark.parametrize("name", list(cat.EXACT_CASES))
def test_every_entry_carries_the_bits_of_its_single_call(ctx, name):
    _against_single_calls(ctx, cat.EXACT_CASES[name])


def test_the_asserted_bound_is_within_the_price_contract():
    assert 0.0 < UPPER_REL < 1e-9 and 0.0 < Q_REL < 1e-9


@pytest.mark.parametrize("name", list(cat.TOLERANCE_CASES))
def test_refilled_lanes_reorder_the_sums_and_nothing_else(ctx, name):
    _against_single_calls(ctx, cat.TOLERANCE_CASES[name])


def test_deep_and_far_entries_stop_where_they_should(ctx):
    """the deep in-the-money put stops at date 1 on every path, the far out-of-the-money one never before N: the chain
    simulates every inner path to N, which is what the far entry's own call does"""
    case = cat.EXACT_CASES["gbm-deep-far-N9-i128"]
    outs, info = cc.run_chain(ctx, case)
    N, items = case["N"], case["n_outer"] * case["n_inner"]
    assert outs[0]["inner_path_steps"] == items * N  # one step from every date
    assert outs[1]["inner_path_steps"] == items * N * (N + 1) // 2
    assert outs[0]["n_exercised_lower"] == case["n_lower"] and outs[1]["n_exercised_lower"] == 0
    assert info["inner_path_steps_simulated"] == outs[1]["inner_path_steps"]


@pytest.mark.parametrize("name", list(cat.TWIN_CASES))
def test_identical_entries_give_identical_outputs(ctx, name):
    case = cat.TWIN_CASES[name]
    outs, info = cc.run_chain(ctx, case)
    for o in outs[1:]:
        for k in cc.EXACT_ALWAYS + cc.UPPER + ("ci_lo", "ci_hi"):
            assert o[k] == outs[0][k], k
        for k in ("betas", "q", "samples"):
            assert np.array_equal(cc.bits(o[k]), cc.bits(outs[0][k])), k
    cc.check_steps(outs, info, same=True)
    cc.compare(case, outs[0], cc.run_single(ctx, case, 0), UPPER_REL, Q_REL)


def test_identical_calls_return_identical_bits_and_leave_the_single_call_alone(ctx):
    case = cat.TOLERANCE_CASES["gbm-E3-N9-i130"]
    before = cc.run_single(ctx, case, 1)
    a, ia = cc.run_chain(ctx, case)
    b, ib = cc.run_chain(ctx, case)
    after = cc.run_single(ctx, case, 1)
    assert ia["inner_path_steps_simulated"] == ib["inner_path_steps_simulated"]
    for x, y in zip(a, b):
        for k in ("q", "samples", "betas"):
            assert np.array_equal(cc.bits(x[k]), cc.bits(y[k])), k
        assert all(x[k] == y[k] for k in cc.EXACT_ALWAYS + cc.UPPER)
    for k in ("q", "samples", "betas"):
        assert np.array_equal(cc.bits(before[k]), cc.bits(after[k])), k


def test_the_facade_returns_the_context_calls_results(ctx):
    from options_model_amd import BoundsResult, HestonBoundsResult, price_american_chain_bounds

    case = cat.EXACT_CASES["gbm-E3-N9-i128"]
    kw = dict(n_lower=case["n_lower"], n_outer=case["n_outer"], n_inner=case["n_inner"], seed=case["seed"],
              stream=case["stream"], ctx=ctx)
    types = ["put" if p else "call" for p in case["puts"]]
    res = price_american_chain_bounds(case["S0"], case["strikes"], case["r"], case["sigma"], case["T"], case["M"], case["N"],
                                      option_types=types, **kw)
    outs, info = cc.run_chain(ctx, case)
    assert len(res) == 3 and all(type(x) is BoundsResult for x in res)
    for x, o, ot in zip(res, outs, types):
        assert (x.lower, x.upper, x.se_upper, x.inner_path_steps, x.option_type) == (o["lower"], o["upper"], o["se_upper"],
                                                                                     o["inner_path_steps"], ot)
        assert np.array_equal(x.betas, o["betas"])
    assert res.inner_path_steps_simulated == info["inner_path_steps_simulated"] and res.n_groups == 1
    assert set(res.timings_ms) == {"fit", "lower", "upper", "total"}
    h = cat.EXACT_CASES["heston-E2-N9-i64"]
    hres = price_american_chain_bounds(h["S0"], h["strikes"], h["r"], None, h["T"], h["M"], h["N"],
                                       option_types=["put" if p else "call" for p in h["puts"]], model="Heston",
                                       heston_params={k: h[k] for k in cc.HP_KEYS}, n_lower=h["n_lower"], n_outer=h["n_outer"],
                                       n_inner=h["n_inner"], seed=h["seed"], stream=h["stream"], ctx=ctx)
    houts, _ = cc.run_chain(ctx, h)
    assert all(type(x) is HestonBoundsResult for x in hres)
    assert [x.upper for x in hres] == [o["upper"] for o in houts]


def test_the_entry_point_refuses_what_is_out_of_scope(ctx):
    case = cat.EXACT_CASES["gbm-E2-N8-i64"]
    p = cc.params_of(case)
    kw = dict(n_lower=64, n_outer=4, n_inner=4)
    with pytest.raises(ValueError, match="1 .. 256 entries"):
        ctx.price_american_chain_bounds(p, [], **kw)
    with pytest.raises(ValueError, match="exercise_every must be 0"):
        ctx.price_american_chain_bounds(p, [100.0, 90.0], exercise_every=[0, 2], **kw)
    for key, value in (("bounds_exercise_every", 2), ("bounds_control_variate", 1), ("bounds_suboptimality", 1)):
        ctx.set_option(key, value)
        try:
            with pytest.raises(ValueError, match="take none of the options"):
                ctx.price_american_chain_bounds(p, [100.0], **kw)
        finally:
            ctx.set_option(key, 0)
    h = cc.params_of(cat.EXACT_CASES["heston-E2-N9-i64"])
    h.heston_scheme = 3
    with pytest.raises(ValueError, match="reference or the full-truncation scheme"):
        ctx.price_american_chain_bounds(h, [100.0], **kw)
    with pytest.raises(ValueError, match="needs a betas table"):
        ctx.price_american_chain_bounds(p, [100.0], policy=3, **kw)
    outs, _ = ctx.price_american_chain_bounds(p, [100.0], **kw)  # and the context still serves
    assert outs[0]["lower"] > 0.0


def test_c_host_example_prints_eight_brackets_that_hold_their_single_calls(tmp_path, ctx):
    """examples/american_chain_bounds.c: a plain C host brackets eight puts through the ABI, each beside its own single call"""
    import os
    import re
    import shutil
    import subprocess

    from options_model_amd import _build
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_chain_bounds"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_chain_bounds.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    out = subprocess.run([str(exe), "9", "4096", "64", "130"], check=True, capture_output=True, text=True, timeout=120).stdout
    rows = re.findall(r"^put K =\s*([0-9.]+)\s+chain \[([0-9.]+), ([0-9.]+)\].*single \[([0-9.]+), ([0-9.]+)\]\s+holds it: (\w+)",
                      out, flags=re.M)
    assert len(rows) == 8 and "8 of 8 chain brackets hold their single-call bracket" in out
    assert [float(r[0]) for r in rows] == [round(80.0 + 40.0 * i / 7.0, 3) for i in range(8)]
    for K, lo, up, lo1, up1, holds in rows:
        assert holds == "yes" and lo == lo1  # (at these sizes the two estimates' noise exceeds the gap: no order between them)
        assert abs(float(up) - float(up1)) <= 1e-6  # (six printed digits; the program itself checks 1.2e-15)
