"""What tests/test_gpu_greeks.py and the Greeks sweep of tests/test_gpu_fuzz.py share: the matrix a pricing stores, and the
comparison of omc_price_american_greeks with the numpy restatement (tests/helpers/greeks_ref.py).  TEST INFRASTRUCTURE ONLY.

Agreement: exercise counts of the three scenarios identical -- unless the restatement shows at least as many decisions
taken within 1e-10 K of the continuation value (ties: either branch is worth the same, and the restatement's non-fused
arithmetic may take the other one) -- and every Greek, price_up and price_down to rel 1e-9 / abs 1e-12."""
import math

VALS = ("price", "delta", "gamma", "vega", "rho", "theta", "price_up", "price_down")


def stored(ctx, p):
    """the full matrix the pricing stores (fold_antithetic 0, or Heston, or no antithetic pairs)"""
    if p.model == 1:
        return ctx.heston_paths(p.n_paths, p.n_steps, p.S0, p.r, p.T, p.v0, p.kappa, p.theta, p.xi, p.rho, p.seed,
                                p.stream, p.pair_offset, scheme=p.heston_scheme)
    return ctx.gbm_paths(p.n_paths, p.n_steps, p.S0, p.r, p.sigma, p.T, p.seed, p.stream, p.pair_offset,
                         antithetic=bool(p.antithetic))


def stored_half(ctx, p):
    """the first partners' half matrix of folded storage (GBM, antithetic pairs)"""
    return ctx.gbm_paths(p.n_paths // 2, p.n_steps, p.S0, p.r, p.sigma, p.T, p.seed, p.stream, p.pair_offset,
                         antithetic=False)


def close(a, b, rel=1e-9, abs_=1e-12):
    return abs(a - b) <= max(rel * abs(b), abs_)


def agrees(d, ref, p):
    """Asserts the agreement above -> True when the values were compared, False when a tie went the other way (the counts
    differ by no more than the restatement's ties, and the values then move by those paths' share: not compared)."""
    counts = [(d["n_exercised"], ref["n_exercised"]), (d["n_exercised_up"], ref["n_exercised_up"]),
              (d["n_exercised_down"], ref["n_exercised_down"])]
    exact = all(a == b for a, b in counts)
    for (a, b), ties in zip(counts, ref["ties"]):
        assert abs(a - b) <= ties, (counts, ref["ties"])
    if not exact:  # a tie went the other way: the values move by that path's share only
        return False
    for k in VALS:
        if p.model == 1 and k in ("vega", "rho", "theta"):
            assert math.isnan(d[k]) and math.isnan(d["se_" + k])
            continue
        assert close(d[k], ref[k]), (k, d[k], ref[k])
        if k not in ("price", "price_up", "price_down"):
            assert close(d["se_" + k], ref["se_" + k], rel=1e-6), (k, d["se_" + k], ref["se_" + k])
    return True
