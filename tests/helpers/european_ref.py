"""European sums and standard errors restated in float64 (numpy + math.fsum, no GPU).  TEST INFRASTRUCTURE ONLY.

What the three kernel families that return European estimators share (block_reduce8, a fixed-order finalize, the host's
mean_and_se of options_model_amd/csrc/omc_ctx.h), restated term by term on float32 terminal spots:

  terminal_body + lsm_finalize (omc_price_european)        terms max(payoff, 0) * df, sums of them and of their squares
  barrier_paths_body + barrier_finalize_kernel             the same terms, split by the path's hit flag
  payoff_chunk_body + payoff_final_kernel (strikes)        RAW payoffs; the host multiplies mean and se by df afterwards

The standard error is the documented one (include/omc.h): sqrt(max(E[x^2] - E[x]^2, 0) / n_paths), antithetic partners
counted as independent paths.  The comparison functions assert that formula; they do not pick a better one.

The layout constants of the kernels (LAYOUT) and the functions that name the layout a path count lands on are here as
well: tests/test_european_ref_cpu.py derives from them what the shape lists of tests/test_gpu_european_sums.py must hold.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)  # unit roundoff of float64

# kBlock, kMaxLsmBlocks (omc_kernels.h), kPayChunk (omc_paths.hip), lanes of a wave
LAYOUT = dict(block=256, max_blocks=1024, pay_chunk=4096, wave=64)


# ------------------------------------------------------------------ the restatement
def terms(ST, K, df, is_put, discount_terms):
    """float64 terms as the kernels build them: p = K - (double)s or (double)s - K, p = p > 0 ? p : 0, and -- where the
    kernel discounts per term (terminal_body's add_payoff, the barrier body's add) -- p = p > 0 ? p * df : 0."""
    s = np.asarray(ST, np.float32).astype(np.float64)
    p = (K - s) if is_put else (s - K)
    p = np.where(p > 0.0, p, 0.0)
    if discount_terms:
        p = np.where(p > 0.0, p * df, 0.0)
    return p


def _sums_of(p):
    p = np.ascontiguousarray(p, np.float64).ravel()
    s = math.fsum(p)
    return dict(sum=s, sumsq=math.fsum(p * p), n_zero=int(np.count_nonzero(p == 0.0)), sum_abs=s, n_paths=int(p.size))


def sums(ST, K, df, is_put, discount_terms):
    """-> dict(sum, sumsq, n_zero, sum_abs, n_paths) of the terms of `terms`: sum and sumsq by math.fsum (the exact sum,
    rounded once); the terms are non-negative, so sum_abs is sum."""
    return _sums_of(terms(ST, K, df, is_put, discount_terms))


def mean_se(sum_, sumsq, M):
    """mean_and_se (omc_ctx.h): mean = sum / M, var = sumsq / M - mean^2 clamped at 0, se = sqrt(var / M)."""
    mean = sum_ / M
    var = sumsq / M - mean * mean
    return mean, math.sqrt((var if var > 0.0 else 0.0) / M)


def barrier_sums(V_T, hit, K, df, is_put):
    """The five quantities of omc_barrier_result from the REAL terminal spots V_T and a boolean `hit` per path: knock-out
    where the path never hit, knock-in where it hit.  Also the sums they come from (out / in: dicts of `sums`) and n_hit."""
    hit = np.asarray(hit, bool)
    p = terms(V_T, K, df, is_put, True)
    assert hit.shape == p.shape
    M = p.size
    out, in_ = _sums_of(np.where(hit, 0.0, p)), _sums_of(np.where(hit, p, 0.0))
    euro_out, euro_out_se = mean_se(out["sum"], out["sumsq"], M)
    euro_in, euro_in_se = mean_se(in_["sum"], in_["sumsq"], M)
    n_hit = int(np.count_nonzero(hit))
    return dict(euro_out=euro_out, euro_out_se=euro_out_se, euro_in=euro_in, euro_in_se=euro_in_se, hit_prob=n_hit / M,
                out=out, n_hit=n_hit, **{"in": in_})


# ------------------------------------------------------------------ comparisons with derived bounds
def sums_close(dev, ref, sum_abs, M):
    """assert |dev - ref| <= 2 M 2^-53 sum_abs   (evaluated exactly, in rationals; dev may be a Fraction).

    Derivation (the bound tests/test_gpu_generator_widths.py::same_pricing derives): `ref` is the exact sum of the M
    reference terms rounded once (fsum): u sum_abs, u = 2^-53.  The device adds the same M terms in float64 in SOME order
    -- per lane, a wave tree, a workgroup tree, a finalize loop --: whatever the order, M - 1 additions, each partial sum
    bounded by sum_abs since the terms are non-negative, so at most (M - 1) u sum_abs to first order (Higham, Accuracy and
    Stability of Numerical Algorithms, 4.2).  A term may itself carry one rounding the reference's does not carry in the
    same way -- the square p * p is rounded on the host and may be fused into `acc += p * p` on the device --: u per term,
    u sum_abs in all.  Together (M + 1) u sum_abs.  A caller that recovers the sum from a mean (sum / M, times df for the
    strike kernels) adds at most 2 u: (M + 3) u <= 2 M u from M = 3; at M = 2 the division by M is exact and the sum is
    ONE addition: 1 + 1 + 1 + 1 = 4 u = 2 M u.  The second-order terms are below M^2 u^2 < 1e-4 u at every M the library
    accepts.  An error of the reduction -- a lost or doubled term -- moves the sum by about sum_abs / M, 1 / (2 M^2 u)
    = 1.6e4 times the bound at M = 524,802."""
    M = int(M)
    bound = 2 * M * U * Fraction(sum_abs)
    miss = abs(Fraction(dev) - Fraction(ref))
    assert miss <= bound, f"sum misses by {float(miss):.3e}, bound {float(bound):.3e} (dev {float(dev)!r}, ref {ref!r}, M {M})"


def se_close(se_dev, sum_ref, sumsq_ref, M, scale=1.0):
    """Compares VARIANCES, so that cancellation in E[x^2] - E[x]^2 needs no case-by-case tolerance:

        | M (se_dev / scale)^2 - var_ref | <= 4 M 2^-53 (sumsq_ref / M + 2 mean_ref^2) + 4 2^-53 var_ref

    with mean_ref = sum_ref / M, var_ref = max(sumsq_ref / M - mean_ref^2, 0) evaluated exactly from the reference sums,
    and exactly se_dev == 0.0 where every reference term is 0 (sumsq_ref == 0).  scale: what the host multiplied the
    standard error by afterwards (df for the strike kernels; for omc_result.std = sqrt(var), scale = sqrt(M)); the left
    side is formed in extended precision (np.longdouble), whose roundings are 2^-11 of float64's.

    Derivation.  By sums_close the device's sums miss the reference's by at most 2 M u of themselves.  The device forms
    mean = fl(s / M), var = fl(fl(s2 / M) - fl(mean^2)): s2 / M inherits (2 M + 1) u (s2 / M); mean inherits (2 M + 1) u,
    its square twice that plus its own rounding, (4 M + 3) u mean^2.  Both are covered by 4 M u (s2 / M + 2 mean^2) from
    M = 1 with (2 M - 1) u (s2 / M) + (4 M - 3) u mean^2 to spare.  What remains is relative to the variance itself: the
    subtraction u, the division by M u, the square root u (2 u on its square), a multiplication by df u (2 u): at most
    6 u var, of which 4 u var is the second term and the rest is inside the spare (s2 / M >= var, so the spare is at
    least 3 u var at M = 2).  A clamped variance (device 0, reference tiny or the reverse) is covered the same way: both
    lie within the first term of the exact value.  An M - 1 in place of M moves the variance by var / M, at M = 524,802
    about 1e3 bounds; a square added once per pair instead of once per partner halves E[x^2]."""
    M = int(M)
    if sumsq_ref == 0.0:
        assert se_dev == 0.0, f"every reference term is 0, the device's standard error is {se_dev!r}"
        return
    mean = Fraction(sum_ref) / M
    ex2 = Fraction(sumsq_ref) / M
    var = max(ex2 - mean * mean, Fraction(0))
    bound = 4 * M * U * (ex2 + 2 * mean * mean) + 4 * U * var
    q = np.longdouble(se_dev) / np.longdouble(scale)
    lhs = np.longdouble(M) * q * q
    var_hi = float(var)
    miss = abs(float(lhs - (np.longdouble(var_hi) + np.longdouble(float(var - Fraction(var_hi))))))
    assert miss <= float(bound), (f"variance misses by {miss:.3e}, bound {float(bound):.3e} "
                                  f"(se {se_dev!r}, scale {float(scale)!r}, reference variance {float(var)!r}, M {M})")


# ------------------------------------------------------------------ which layout a path count lands on
def barrier_vec(M):
    """barrier_vec (omc_barrier.hip): four pairs per thread where the pair count is a multiple of 4, else one."""
    return 4 if (M // 2) % 4 == 0 else 1


def barrier_blocks(M):
    per = LAYOUT["block"] * barrier_vec(M)
    return max(1, -(-(M // 2) // per))


def terminal_layout(M, antithetic=True):
    """-> (work items P, workgroups launched, lanes of the grid-stride loop's second trip, lanes of the last workgroup)"""
    B = LAYOUT["block"]
    P = M // 2 if antithetic else M
    nblk = min(max(1, -(-P // B)), LAYOUT["max_blocks"])
    second = max(0, min(P - nblk * B, nblk * B))
    return P, nblk, second, (P - (nblk - 1) * B if P <= nblk * B else B)


def barrier_layout(M):
    """-> (VEC, workgroups = partials of the finalize, threads of the last workgroup with pairs, finalize trips)"""
    B = LAYOUT["block"]
    vec, nblk = barrier_vec(M), barrier_blocks(M)
    threads = M // 2 // vec
    return vec, nblk, threads - (nblk - 1) * B, -(-nblk // B)


def strikes_layout(M):
    """-> (chunks, spots of the last chunk)"""
    C = LAYOUT["pay_chunk"]
    n = max(1, -(-M // C))
    return n, M - (n - 1) * C
