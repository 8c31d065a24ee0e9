"""What the multi-asset bound tests share (omc_price_american_basket_bounds).  TEST INFRASTRUCTURE ONLY.

The device's own spots for the numpy restatement of tests/helpers/bounds_ref.py, all from omc_price_american_basket calls at
the documented Philox coordinates (the library has no test-only entry point):
  lower paths   S_keep of a call with n_paths = n_lower at stream_lower, pair_offset 0
  outer paths   S_keep and assets_keep of a call with n_paths = n_outer at stream_outer, pair_offset 0
  inner paths   of item (i, t): rows 0 .. N-t of the S_keep of a RESTART call -- the basket with S0[k] = A_k[t][i],
                n_paths = n_inner at stream_inner, pair_offset = (i (N+1) + t) n_inner / 2
and the seeded case generator of tests/test_gpu_basket_bounds_fuzz.py, which needs no GPU (test_basket_bounds_cases_cpu.py).
"""
from __future__ import annotations

import numpy as np

from helpers import bounds_ref as br
from options_model_amd import _ffi

KINDS = ("basket", "best-of", "worst-of")
POLICIES = ("textbook", "two_pass", "reference", "given")


RHO3 = np.array([[1.0, 0.5, 0.2], [0.5, 1.0, -0.3], [0.2, -0.3, 1.0]])


def equi(d, c):
    return np.full((d, d), c) + (1.0 - c) * np.eye(d)


def unequal_basket(d, kind):
    """unequal spots, sigmas, yields and weights; a non-trivial correlation"""
    S0 = [96.0 + 3.0 * k for k in range(d)]
    sig = [0.16 + 0.03 * k for k in range(d)]
    q = [0.01 * ((k * 3) % 5) for k in range(d)]
    w = [(0.7 + 0.1 * k) / d for k in range(d)] if kind == "basket" else [1.04 - 0.02 * k for k in range(d)]
    rho = {2: np.array([[1.0, -0.4], [-0.4, 1.0]]), 3: RHO3}.get(d, equi(d, 0.3))
    return _ffi.make_basket(S0, sig, q, w, rho, kind)


def with_fields(s, **kw):
    """a copy of a ctypes structure with some fields replaced"""
    c = type(s).from_buffer_copy(bytes(s))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def index_and_assets(ctx, p, b, assets=True):
    """-> (index matrix [N+1][M], asset matrices [d][N+1][M] or None) of omc_price_american_basket(p, b)"""
    d, N, M = int(b.n_assets), int(p.n_steps), int(p.n_paths)
    keep = ctx.empty((N + 1, M), np.float32)
    akeep = ctx.empty((d, N + 1, M), np.float32) if assets else None
    ctx.price_american_basket(p, b, S_keep=keep, assets_keep=akeep)
    S = keep.to_host()
    A = akeep.to_host() if assets else None
    keep.free()
    if assets:
        akeep.free()
    return S, A


def fitted_table(ctx, p, b, policy):
    """omc_lsm_poly's fits with semantics `policy` on the device's own index matrix of (p, b) -> betas4 [N+1][4]"""
    N, M = int(p.n_steps), int(p.n_paths)
    keep = ctx.empty((N + 1, M), np.float32)
    ctx.price_american_basket(p, b, S_keep=keep)
    d = ctx.lsm_poly(keep, p.K, p.r, p.T, bool(p.is_put), policy)
    keep.free()
    t = np.zeros((N + 1, 4))
    t[:, :3], t[:, 3] = d["betas"], d["nitm"]
    return t


def device_spots(ctx, p, b, n_lower, n_outer, n_inner, streams=None):
    """-> dict Sl (lower index paths), So, Ao (outer index / assets) and inner(i, t) -> [N - t + 1][n_inner] index spots"""
    N, d = int(p.n_steps), int(b.n_assets)
    s_lo, s_out, s_in = streams or (p.stream + 1, p.stream + 2, p.stream + 3)
    Sl, _ = index_and_assets(ctx, with_fields(p, n_paths=n_lower, stream=s_lo, pair_offset=0), b, assets=False)
    So, Ao = index_and_assets(ctx, with_fields(p, n_paths=n_outer, stream=s_out, pair_offset=0), b)
    H = n_inner // 2
    keep = ctx.empty((N + 1, n_inner), np.float32)

    def inner(i, t):
        rb = with_fields(b)
        for k in range(d):
            rb.S0[k] = float(Ao[k, t, i])
        ctx.price_american_basket(with_fields(p, n_paths=n_inner, stream=s_in, pair_offset=(i * (N + 1) + t) * H), rb,
                                  S_keep=keep)
        return keep.to_host()[:N - t + 1]

    return dict(Sl=Sl, So=So, Ao=Ao, inner=inner, free=keep.free)


def check_against_restatement(ctx, p, b, dev, n_lower, n_outer, n_inner, rtol=1e-12):
    """The device's result dict `dev` (want_q, want_samples) against bounds_ref on the device's own spots: no ties, equal
    counts, q / samples / bounds at rtol (atol rtol K, as tests/test_gpu_bounds.py)."""
    K, is_put = float(p.K), bool(p.is_put)
    sp = device_spots(ctx, p, b, n_lower, n_outer, n_inner)
    try:
        lo = br.lower_bound(sp["Sl"], K, p.r, p.T, is_put, dev["betas"])
        up = br.upper_bound(sp["So"], sp["inner"], K, p.r, p.T, is_put, dev["betas"])
    finally:
        sp["free"]()
    assert lo["ties"] == 0 and up["ties"] == 0  # numpy's decisions are the device's
    assert dev["n_exercised_lower"] == lo["n_exercised"]
    assert dev["inner_path_steps"] == up["inner_path_steps"]
    np.testing.assert_allclose(dev["q"], up["q"], rtol=rtol, atol=rtol * K)
    np.testing.assert_allclose(dev["samples"], up["samples"], rtol=rtol, atol=rtol * K)
    for k in ("lower", "se_lower"):
        np.testing.assert_allclose(dev[k], lo[k], rtol=rtol, atol=rtol * K, err_msg=k)
    for k in ("upper", "se_upper"):
        np.testing.assert_allclose(dev[k], up[k], rtol=rtol, atol=rtol * K, err_msg=k)
    assert dev["ci_lo"] == dev["lower"] - 1.96 * dev["se_lower"] and dev["ci_hi"] == dev["upper"] + 1.96 * dev["se_upper"]
    assert (dev["n_lower"], dev["n_outer"], dev["n_inner"]) == (n_lower, n_outer, n_inner)
    return lo, up


def random_correlation(rng, d):
    """a well-conditioned random correlation matrix: normalised G G^T + d I"""
    G = rng.standard_normal((d, d))
    C = G @ G.T + d * np.eye(d)
    s = 1.0 / np.sqrt(np.diag(C))
    C = C * s[:, None] * s[None, :]
    C = 0.5 * (C + C.T)
    np.fill_diagonal(C, 1.0)
    return C


# ---------------------------------------------------------------------------------------------- the fuzz cases
N_INNER = (2, 64, 130, 200)


def fuzz_cases(n, seed=20260417):
    """n seeded cases of the fuzz sweep, as plain dicts: d in 1 .. 8 and the three kinds (both cycled, so a sweep of 24 or
    more draws every combination's marginals and one of 8 every d), N in 1 .. 13, n_inner of N_INNER, a ragged n_outer,
    a policy (every fourth case a given table with n = 0 holes), put / call, the float64 fallback on some.  refill: more
    inner pairs than a wave has lanes."""
    rng = np.random.default_rng(seed)
    perm_d = rng.permutation(8)
    out = []
    for c in range(n):
        d = int(perm_d[c % 8]) + 1
        kind = KINDS[(c + c // 3) % 3]
        n_inner = N_INNER[3 - c % 4] if c % 3 else int(rng.choice((130, 200)))  # at least a third refill
        N = int(rng.integers(1, 14))
        case = dict(d=d, kind=kind, N=N, n_inner=n_inner, n_outer=2 * int(rng.integers(1, 12)),
                    n_lower=2 * int(rng.integers(100, 700)), M=2 * int(rng.integers(300, 1500)),
                    is_put=bool(rng.integers(0, 2)), policy=POLICIES[c % 4], irr_every=int(rng.choice((0, 0, 1, 2, 3))),
                    seed=int(rng.integers(1, 1 << 31)), stream=int(rng.integers(0, 50)),
                    S0=[float(x) for x in rng.uniform(85.0, 115.0, d)], sigma=[float(x) for x in rng.uniform(0.1, 0.4, d)],
                    q=[float(x) for x in rng.uniform(0.0, 0.08, d)], rho=random_correlation(rng, d), T=float(rng.uniform(0.5, 3.0)))
        w = rng.uniform(0.5, 1.5, d)
        case["w"] = [float(x) for x in (w / w.sum() if kind == "basket" else w / w.mean())]
        holes = rng.random(N + 1) < 0.3  # dates of a given table where nobody was in the money: n = 0
        case["holes"] = [bool(x) for x in holes]
        case["refill"] = n_inner // 2 > 64
        out.append(case)
    return out


def fuzz_given_table(ctx, p, b, holes):
    """a policy from other paths (stream 9 of p's seed), textbook fits, with n = 0 on the dates `holes` marks"""
    t = fitted_table(ctx, with_fields(p, n_paths=2048, stream=9, pair_offset=0), b, "textbook")
    t[np.asarray(holes), 3] = 0.0
    return t


def fuzz_params(case):
    p = _ffi.make_params(model="gbm", is_put=case["is_put"], semantics="two_pass", n_paths=case["M"], n_steps=case["N"],
                         S0=case["S0"][0], K=100.0, r=0.05, sigma=case["sigma"][0], T=case["T"], seed=case["seed"],
                         stream=case["stream"])
    b = _ffi.make_basket(case["S0"], case["sigma"], case["q"], case["w"], case["rho"], case["kind"])
    return p, b
