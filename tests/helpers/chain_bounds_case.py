"""What the chain price-bound tests share (omc_price_american_chain_bounds).  TEST INFRASTRUCTURE ONLY.

A case is a plain dict: the law (model "gbm" or "heston", scheme 0 / 1, the market, the Heston parameters), the sizes, the seed
and stream, the chain (strikes, puts), the policy, the kind of every entry's table with policy "given", and the value of the
context option "pass2_tables_irregular_every".  run_chain / run_single call the chain and one entry's own single call on a
context; compare holds the contract of include/omc_chain_bounds.h between them.  fuzz_cases is the seeded generator of
tests/test_gpu_chain_bounds_fuzz.py; it needs no GPU (tests/test_chain_bounds_cpu.py checks its limits).
"""
from __future__ import annotations

import numpy as np

from options_model_amd import _ffi

HP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
HP_KEYS = ("v0", "kappa", "theta", "xi", "rho")
POLICIES = ("textbook", "two_pass", "reference", "given")
CAP = _ffi.CHAIN_BOUNDS_MAX
EXACT_INNER = 128  # n_inner up to which no lane of the inner sweep is refilled: Q^ carries the single call's bits

# The measured worst deviations of a chain entry from its own single call where lanes are refilled (n_inner > 128), on an
# MI355X over chain_bounds_catalogue.TOLERANCE_CASES and the refilling ones of 200 seeded fuzz cases -- 87 cases, every entry
# of each (OMC_FUZZ_SCALE=20 tools/time_chain_bounds.py --deviation prints them): upper 2.997e-16 relative, q 2.920e-16 of
# max|q|, the order of float64 sums of at most 256 non-negative terms per lane.  The tests assert 4x these, far below the
# README's 1e-9.
MEASURED_UPPER_REL = 3.0e-16
MEASURED_Q_REL = 3.0e-16   # of max|q|


def make_case(**kw):
    case = dict(model="gbm", scheme=0, S0=100.0, r=0.05, sigma=0.2, T=1.0, N=8, M=8192, n_lower=4096, n_outer=64, n_inner=64,
                seed=42, stream=0, strikes=[100.0], puts=[True], policy="textbook", given=None, irr_every=0, **HP)
    case.update(kw)
    if isinstance(case["puts"], bool):
        case["puts"] = [case["puts"]] * len(case["strikes"])
    assert len(case["puts"]) == len(case["strikes"])
    return case


def params_of(case, e=0):
    """omc_params of the case with entry e's strike and side (what that entry's single call is handed)"""
    kw = dict(is_put=case["puts"][e], semantics="two_pass", antithetic=True, n_paths=case["M"], n_steps=case["N"],
              S0=case["S0"], K=case["strikes"][e], r=case["r"], T=case["T"], seed=case["seed"], stream=case["stream"])
    if case["model"] == "heston":
        return _ffi.make_params(model="heston", heston_scheme=case["scheme"], sigma=0.0, **kw, **{k: case[k] for k in HP_KEYS})
    return _ffi.make_params(sigma=case["sigma"], **kw)


def given_tables(case):
    """The entries' tables of policy "given", [E][N+1][4], from the case alone (no device): kind "zero" is the all-zero table
    (never stops before N), "flat" stops wherever the payoff exceeds a fixed fraction of the strike, "holes" is "flat" with
    n = 0 on every third date, "curve" a quadratic in u = s / K - 1."""
    if case["policy"] != "given":
        return None
    N, kinds = case["N"], case["given"]
    out = np.zeros((len(case["strikes"]), N + 1, 4))
    for e, (K, kind) in enumerate(zip(case["strikes"], kinds)):
        for t in range(1, N):
            if kind == "zero" or (kind == "holes" and t % 3 == 0):
                continue
            frac = 0.02 + 0.1 * (N - t) / N
            out[e, t] = (frac * K, 0.0, 0.0, 100.0) if kind != "curve" else (frac * K, -0.3 * K, 0.5 * K, 100.0)
    return out


def _sizes(case):
    return dict(policy=case["policy"], n_lower=case["n_lower"], n_outer=case["n_outer"], n_inner=case["n_inner"],
                want_q=True, want_samples=True)


class irregular:
    """option "pass2_tables_irregular_every" = the case's value for the calls inside, 0 after them"""

    def __init__(self, ctx, case):
        self.ctx, self.k = ctx, case["irr_every"]

    def __enter__(self):
        self.ctx.set_option("pass2_tables_irregular_every", self.k)

    def __exit__(self, *exc):
        self.ctx.set_option("pass2_tables_irregular_every", 0)


def run_chain(ctx, case):
    """-> (list of per-entry dicts with q and samples, info dict)"""
    with irregular(ctx, case):
        return ctx.price_american_chain_bounds(params_of(case), case["strikes"], case["puts"], betas=given_tables(case),
                                               **_sizes(case))


def run_single(ctx, case, e):
    """entry e's own call: omc_price_american_bounds, or omc_price_american_bounds_heston with regressors spot"""
    tabs = given_tables(case)
    call = ctx.price_american_bounds_heston if case["model"] == "heston" else ctx.price_american_bounds
    with irregular(ctx, case):
        return call(params_of(case, e), betas=None if tabs is None else tabs[e], **_sizes(case))


EXACT_ALWAYS = ("lower", "se_lower", "n_exercised_lower", "inner_path_steps", "n_lower", "n_outer", "n_inner")
UPPER = ("upper", "se_upper")


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def deviation(got, ref):
    """-> (relative deviation of upper, worst deviation of q against max|q|) of a chain entry from its single call"""
    up = abs(got["upper"] - ref["upper"]) / max(abs(ref["upper"]), 1e-300)
    qmax = float(np.max(np.abs(ref["q"]), initial=0.0))
    dq = float(np.max(np.abs(got["q"] - ref["q"]), initial=0.0)) / max(qmax, 1e-300)
    return up, dq


def compare(case, got, ref, upper_rel=None, q_rel=None):
    """One chain entry `got` against its own single call `ref` (contract items 1 - 3).  Exact always: betas, lower, se_lower,
    n_exercised_lower, inner_path_steps.  n_inner <= 128: q, samples, upper, se_upper exact too.  Beyond: upper within
    upper_rel relative, q within q_rel of max|q|, samples and se_upper within the walk's share of that (2 N terms of Q^)."""
    assert np.array_equal(bits(got["betas"]), bits(ref["betas"])), "betas"
    for k in EXACT_ALWAYS:
        if isinstance(ref[k], float):
            assert bits(got[k]) == bits(ref[k]), (k, got[k], ref[k])
        else:
            assert got[k] == ref[k], (k, got[k], ref[k])
    if case["n_inner"] <= EXACT_INNER:
        assert np.array_equal(bits(got["q"]), bits(ref["q"])), "q"
        assert np.array_equal(bits(got["samples"]), bits(ref["samples"])), "samples"
        for k in UPPER:
            assert bits(got[k]) == bits(ref[k]), (k, got[k], ref[k])
        return 0.0, 0.0
    up, dq = deviation(got, ref)
    print(f"chain entry vs single call, n_inner {case['n_inner']}: upper rel {up:.3e}, q / max|q| {dq:.3e}")
    assert up <= upper_rel, ("upper", up, upper_rel)
    assert dq <= q_rel, ("q", dq, q_rel)
    return up, dq


def check_steps(outs, info, same=False):
    """contract item 5: the simulated steps against the entries' own counts; the groups"""
    steps = [o["inner_path_steps"] for o in outs]
    sim, per = info["inner_path_steps_simulated"], info["entries_per_group"]
    groups = [steps[i:i + per] for i in range(0, len(steps), per)]
    assert info["n_groups"] == len(groups)
    assert sum(max(g) for g in groups) <= sim <= sum(steps), (sim, steps)  # per group: at least its largest entry's
    assert max(steps) <= sim
    if same:
        assert sim == sum(g[0] for g in groups), (sim, steps)


# ---------------------------------------------------------------------------------------------- the fuzz cases
LIMITS = dict(N=(1, 13), n_outer=(2, 40), n_lower=(200, 1400), M=(600, 3000), E=(1, CAP + 2))
N_INNER = (2, 64, 128, 130, 512)
GIVEN_KINDS = ("zero", "flat", "holes", "curve")


def fuzz_cases(n, seed=20261021):
    """n seeded cases: N in 1 .. 13, n_inner of N_INNER (two in five with refills), a ragged even n_outer up to 40, GBM and
    both Heston schemes, 1 .. cap + 2 entries with mixed sides and strikes at 0.5 .. 1.6 of the spot (so some entries stop at
    once and some never), every policy (given tables of every kind), the float64 fallback on some."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        E = int(rng.integers(LIMITS["E"][0], LIMITS["E"][1] + 1))
        S0 = 100.0 * float(rng.uniform(0.8, 1.25))
        policy = POLICIES[c % 4]
        kappa, theta = float(rng.uniform(0.5, 4.0)), float(rng.uniform(0.01, 0.09))
        case = make_case(model=("gbm", "heston", "heston")[c % 3], scheme=(c // 3) % 2, S0=S0, r=float(rng.uniform(0.0, 0.08)),
                         sigma=float(rng.uniform(0.1, 0.5)), T=float(rng.uniform(0.5, 3.0)),
                         N=int(rng.integers(LIMITS["N"][0], LIMITS["N"][1] + 1)),
                         M=2 * int(rng.integers(LIMITS["M"][0] // 2, LIMITS["M"][1] // 2 + 1)),
                         n_lower=2 * int(rng.integers(LIMITS["n_lower"][0] // 2, LIMITS["n_lower"][1] // 2 + 1)),
                         n_outer=2 * int(rng.integers(LIMITS["n_outer"][0] // 2, LIMITS["n_outer"][1] // 2 + 1)),
                         n_inner=N_INNER[c % 5], seed=int(rng.integers(1, 1 << 31)), stream=int(rng.integers(0, 50)),
                         strikes=[S0 * float(rng.uniform(0.5, 1.6)) for _ in range(E)],
                         puts=[bool(rng.integers(0, 2)) for _ in range(E)], policy=policy,
                         given=[GIVEN_KINDS[int(rng.integers(0, 4))] for _ in range(E)] if policy == "given" else None,
                         irr_every=int(rng.choice((0, 0, 1, 2, 3))), v0=float(rng.uniform(0.01, 0.09)), kappa=kappa,
                         theta=theta, xi=float(np.sqrt(2.0 * kappa * theta)) * float(rng.uniform(0.3, 2.0)),
                         rho=float(rng.uniform(-0.9, 0.5)))
        out.append(case)
    return out


def case_id(c):
    return (f"{c['model']}{c['scheme']}-E{len(c['strikes'])}-N{c['N']}-i{c['n_inner']}-o{c['n_outer']}-{c['policy']}"
            f"-irr{c['irr_every']}")
