"""What the Heston bound tests share (omc_price_american_bounds_heston).  TEST INFRASTRUCTURE ONLY.

The device's own spots for the numpy restatement of tests/helpers/bounds_ref.py, from the generators at the documented
Philox coordinates:
  lower paths   Context.heston_paths(n_lower, ..) at stream_lower, pair_offset 0
  outer paths   Context.heston_paths_sv(n_outer, ..) at stream_outer, pair_offset 0: spots So and variance state Vo
  inner paths   of item (i, t): Context.gbm_normals(n_inner / 2, 2 N, seed, stream_inner, pair_offset = (i (N+1) + t)
                n_inner / 2) -- rows 2(k-1) and 2(k-1)+1 are (z1, z2) of Heston step k: the Heston generator draws one
                Philox block per two steps and uses words (0, 1) and (2, 3), the normals kernel one block per four rows
                -- through Context.heston_paths_from_normals started at (So[t, i], Vo[t, i]), rows 0 .. N-t.  That
                entry point does not validate v0, so a negative scheme-1 state passes; a float32 is exact in its double.
Device and libm sqrt / exp2 differ by an ulp, so the comparison is on the device's own spots, as the GBM tests do it.
And the seeded case generator of tests/test_gpu_heston_bounds_fuzz.py, which needs no GPU (test_heston_bounds_cpu.py).
"""
from __future__ import annotations

import numpy as np

from helpers import bounds_ref as br
from options_model_amd import _ffi

HP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)        # Feller holds: 2 kappa theta = 0.16 > xi^2 = 0.09
HP_CLAMP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=1.0, rho=-0.7)  # the `clamp` golden set: 0.16 < 1, the variance hits 0
POLICIES = ("textbook", "two_pass", "reference", "given")
HP_KEYS = ("v0", "kappa", "theta", "xi", "rho")


def make_params(hp, scheme=0, is_put=True, S0=100.0, K=100.0, r=0.05, T=1.0, N=8, M=4096, seed=42, stream=0):
    return _ffi.make_params(model="heston", heston_scheme=scheme, is_put=is_put, semantics="two_pass", n_paths=M,
                            n_steps=N, S0=S0, K=K, r=r, sigma=0.0, T=T, seed=seed, stream=stream, **hp)


def hp_of(p):
    return [getattr(p, k) for k in HP_KEYS]


def host(a):
    h = a.to_host()
    a.free()
    return h


def inner_from_state(normals, spots, So, Vo, n_inner):
    """inner(i, t) for bounds_ref.upper_bound.  normals(pair_offset, n_pairs) -> [2 N][n_pairs] of stream_inner;
    spots(z1 [N][H], z2 [N][H], s0, v0) -> [N+1][2 H] started at (s0, v0).  Pair j of item (i, t) is generator pair
    (i (N+1) + t) n_inner/2 + j; Heston step k takes rows 2(k-1) and 2(k-1)+1; rows after N - t are dropped."""
    N = So.shape[0] - 1
    H = n_inner // 2

    def inner(i, t):
        z = normals((i * (N + 1) + t) * H, H)
        z1, z2 = np.ascontiguousarray(z[0::2]), np.ascontiguousarray(z[1::2])
        return spots(z1, z2, float(So[t, i]), float(Vo[t, i]))[:N - t + 1]

    return inner


def fitted_table(ctx, p, policy):
    """omc_lsm_poly's fits with semantics `policy` on the device's own Heston paths of p -> betas4 [N+1][4]"""
    S = ctx.heston_paths(int(p.n_paths), int(p.n_steps), p.S0, p.r, p.T, *hp_of(p), p.seed, p.stream, p.pair_offset,
                         int(p.heston_scheme))
    d = ctx.lsm_poly(S, p.K, p.r, p.T, bool(p.is_put), policy)
    S.free()
    t = np.zeros((int(p.n_steps) + 1, 4))
    t[:, :3], t[:, 3] = d["betas"], d["nitm"]
    return t


def given_table(ctx, p, holes=None):
    """a policy from other paths (2048 of stream 9 of p's seed), textbook fits, with n = 0 on the dates `holes` marks"""
    q = type(p).from_buffer_copy(bytes(p))
    q.n_paths, q.stream, q.pair_offset = 2048, 9, 0
    t = fitted_table(ctx, q, "textbook")
    if holes is not None:
        t[np.asarray(holes), 3] = 0.0
    return t


def device_spots(ctx, p, n_lower, n_outer, n_inner, streams=None, cache=False):
    """-> dict Sl (lower paths), So, Vo (outer spots / variance state) and inner(i, t) -> [N - t + 1][n_inner] spots.
    The spots depend on the law, seed and streams of p, not on its payoff or the policy; cache=True computes every item
    once (for cases that several tests share)."""
    N, sch, hp = int(p.n_steps), int(p.heston_scheme), hp_of(p)
    s_lo, s_out, s_in = streams or (p.stream + 1, p.stream + 2, p.stream + 3)
    Sl = host(ctx.heston_paths(n_lower, N, p.S0, p.r, p.T, *hp, p.seed, s_lo, 0, sch))
    Sd, Vd = ctx.heston_paths_sv(n_outer, N, p.S0, p.r, p.T, *hp, p.seed, s_out, 0, sch)
    So, Vo = host(Sd), host(Vd)
    kappa, theta, xi, rho = hp[1:]
    inner = inner_from_state(lambda off, n: host(ctx.gbm_normals(n, 2 * N, p.seed, s_in, off)),
                             lambda z1, z2, s0, v0: host(ctx.heston_paths_from_normals(z1, z2, s0, p.r, p.T, v0, kappa, theta,
                                                                                         xi, rho, sch)),
                             So, Vo, n_inner)
    if cache:
        items = {(i, t): inner(i, t) for i in range(n_outer) for t in range(N)}
        inner = lambda i, t: items[(i, t)]  # noqa: E731
    return dict(Sl=Sl, So=So, Vo=Vo, inner=inner)


def check_against_restatement(p, dev, sp, n_lower, n_outer, n_inner, rtol=1e-12):
    """The device's result dict `dev` (want_q, want_samples) against bounds_ref on the device's own spots `sp`: no ties,
    equal counts, q / samples / bounds at rtol (atol rtol K, as tests/test_gpu_bounds.py)."""
    K, is_put = float(p.K), bool(p.is_put)
    lo = br.lower_bound(sp["Sl"], K, p.r, p.T, is_put, dev["betas"])
    up = br.upper_bound(sp["So"], sp["inner"], K, p.r, p.T, is_put, dev["betas"])
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


# ---------------------------------------------------------------------------------------------- the fuzz cases
N_INNER = (2, 64, 130, 200)


def fuzz_cases(n, seed=20261019):
    """n seeded cases of the fuzz sweep, as plain dicts: N in 1 .. 13, n_inner of N_INNER (at least a third with more
    inner pairs than a wave has lanes: the refill), a ragged even n_outer up to 40, schemes 0 and 1, put / call, a policy
    (every fourth case a given table with n = 0 holes), the float64 fallback on some, random (v0, kappa, theta, xi, rho)
    with every third case violating Feller (2 kappa theta < xi^2), S0 / K in 0.8 .. 1.25."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        n_inner = N_INNER[3 - c % 4] if c % 3 else int(rng.choice((130, 200)))
        N = int(rng.integers(1, 14))
        kappa, theta = float(rng.uniform(0.5, 4.0)), float(rng.uniform(0.01, 0.09))
        bound = float(np.sqrt(2.0 * kappa * theta))  # Feller: xi below it
        xi = bound * float(rng.uniform(1.3, 3.0)) if c % 3 == 2 else bound * float(rng.uniform(0.2, 0.9))
        case = dict(N=N, n_inner=n_inner, n_outer=2 * int(rng.integers(1, 21)), n_lower=2 * int(rng.integers(100, 700)),
                    M=2 * int(rng.integers(300, 1500)), scheme=(c + c // 2) % 2, is_put=bool(rng.integers(0, 2)),
                    policy=POLICIES[c % 4], irr_every=int(rng.choice((0, 0, 1, 2, 3))),
                    seed=int(rng.integers(1, 1 << 31)), stream=int(rng.integers(0, 50)),
                    S0=100.0 * float(rng.uniform(0.8, 1.25)), K=100.0, r=float(rng.uniform(0.0, 0.08)),
                    T=float(rng.uniform(0.5, 3.0)), v0=float(rng.uniform(0.01, 0.09)), kappa=kappa, theta=theta, xi=xi,
                    rho=float(rng.uniform(-0.9, 0.5)))
        case["feller"] = 2.0 * kappa * theta >= xi * xi
        case["holes"] = [bool(x) for x in rng.random(N + 1) < 0.3]  # dates of a given table with n = 0
        case["refill"] = n_inner // 2 > 64
        out.append(case)
    return out


def fuzz_params(case):
    return make_params({k: case[k] for k in HP_KEYS}, scheme=case["scheme"], is_put=case["is_put"], S0=case["S0"],
                       K=case["K"], r=case["r"], T=case["T"], N=case["N"], M=case["M"], seed=case["seed"],
                       stream=case["stream"])
