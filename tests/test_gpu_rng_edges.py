"""The random draws at the edges of their words ("the draws at their edges").

tests/golden/rng_edges.json (tools/mine_rng_edges.py) holds the coordinates -- pair, third counter word, word slot -- at which
the Philox stream of seed 0x9E3779B97F4A7C15, stream 0xDEADBEEF carries a word no random sample reaches: a radius word of 0
or 0xFFFFFF, an angle word on a quarter turn, the largest |z| of 2^29 normals, a jump-count word equal to a Poisson
threshold, a bridge uniform of 0.  Every test here asks the device for exactly those pairs through pair_offset.

  a. normals       gbm_normals at each row, alone and as each lane of a 4-pair call: 4e-6 to the float64 Box-Muller on the
                   fixture's words (the contract's number), finite, |z| <= 5.8870502 + 4e-6, +-0 at radius word 0xFFFFFF
  b. bulk          2^20 pairs x 16 steps against the C oracle: 4e-6, and the same tail counts beyond 3, 4, 4.5 and 5
  c. generators    gbm_paths, heston_paths schemes 0..3 through every tail and radius row, against their own references
                   at their own tolerances, 8 paths (the pair in each lane) and 2 paths
  d. jump counts   price_american_jump where the count word equals a threshold or its predecessor, and at the largest counts
  e. bridge        price_barrier, continuous monitoring, where the bridge uniform is 0, 2^-24 or 1 - 2^-24: bit for bit

tests/test_rng_edges_cpu.py shows that the references alone meet every condition imposed here.
"""
import math
import os

import numpy as np
import pytest

from helpers import barrier_ref as br
from helpers import dividend_ref as dr
from helpers import heston_qe_ref as qe
from helpers import jump_ref as jr
from helpers import rng_edges as re_
from oracle import cpu as orc
from options_model_amd import _ffi
from test_gpu_barrier import K as BK, R as BR, S0 as BS0, SIG as BSIG, T as BT, _barrier, _H, _params as barrier_params, _vanilla
from test_gpu_dividends import RTOL, bits, params as div_params
from test_gpu_jumps import MU, Q, SJ, priced, vanilla_at

pytestmark = pytest.mark.gpu

SEED, STREAM, N = re_.SEED, re_.STREAM, re_.N_STEPS
FX = re_.load()
R0, SIG0, T0 = 0.05, 0.2, 1.0
HP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)  # tests/test_gpu_parity.py's Heston law
REPORT = []  # the measured figures, in the order the tests run (profiles/rng_edges.txt)


def note(line):
    print(line)
    REPORT.append(line)


def host(a):
    h = a.to_host()
    a.free()
    return h


def placements(pair):
    """(pair_offset, n_pairs, lane): the pair alone, then as each lane of a 4-pair call (four pairs per thread)"""
    return [(pair, 1, 0)] + [(pair - j, 4, j) for j in range(4)]


# ------------------------------------------------------------------ a. normals
@pytest.mark.parametrize("cls", ["radius", "angle", "tail"])
def test_normals_at_the_mined_words(ctx, cls):
    worst, fails = 0.0, []
    for r in re_.rows_of(FX, cls):
        ref = re_.reference_normals(r)
        zo = orc.gbm_normals(1, N, SEED, STREAM, r["pair"])[:, 0]
        alone = None
        for off, n_pairs, lane in placements(r["pair"]):
            Z = host(ctx.gbm_normals(n_pairs, N, SEED, STREAM, off))
            assert np.isfinite(Z).all(), (r, off)
            assert np.abs(Z).max() <= re_.Z_MAX + re_.Z_TOL, (r, off, float(np.abs(Z).max()))
            z = Z[:, lane]
            alone = z if alone is None else alone
            assert np.array_equal(bits(z), bits(alone)), (r, off)  # a pair's normals do not depend on its lane
            rest = [t for t in range(N) if t not in ref]
            assert np.abs(z[rest].astype(np.float64) - zo[rest]).max() <= re_.Z_TOL, (r, off)  # the pair's ordinary normals
            for t, want in ref.items():
                err = abs(float(z[t]) - want)
                worst = max(worst, err)
                if err > re_.Z_TOL:
                    fails.append((r["pair"], r["words"], t, float(z[t]), want, err))
                if r["words"][0] == re_.W24:
                    assert z[t] == 0.0, (r, t, float(z[t]))  # sqrt(-0) times anything: +-0 exactly
    note(f"normals, class {cls:6s} {len(re_.rows_of(FX, cls)):3d} rows: worst |z - float64 Box-Muller| {worst:.3e}")
    assert not fails, fails[:5]


# ------------------------------------------------------------------ b. bulk
def test_bulk_normals_and_their_tail_counts_match_the_oracle(ctx):
    P = 1 << 20
    Z = host(ctx.gbm_normals(P, N, SEED, STREAM, 0))
    Zo = orc.gbm_normals(P, N, SEED, STREAM, 0)
    assert np.isfinite(Z).all()
    err = np.abs(Z.astype(np.float64) - Zo)
    note(f"bulk 2^20 pairs x 16: max |dz| against the oracle {err.max():.3e}, largest |z| device {np.abs(Z).max():.4f} oracle {np.abs(Zo).max():.4f}")
    assert err.max() <= re_.Z_TOL
    a, ao = np.abs(Z.astype(np.float64)), np.abs(Zo.astype(np.float64))
    aside = 0
    for thr in (3.0, 4.0, 4.5, 5.0):
        near = (np.abs(a - thr) <= re_.Z_TOL) | (np.abs(ao - thr) <= re_.Z_TOL)
        aside += int(near.sum())
        n_dev, n_orc = int(((a > thr) & ~near).sum()), int(((ao > thr) & ~near).sum())
        note(f"bulk |z| > {thr}: device {n_dev} oracle {n_orc}, set aside {int(near.sum())}")
        assert n_dev == n_orc and n_orc > 0, thr
    assert aside <= 8, aside


# ------------------------------------------------------------------ c. every generator through an extreme normal
def _gbm(ctx, M, off):
    S = host(ctx.gbm_paths(M, N, 100.0, R0, SIG0, T0, SEED, STREAM, off))
    So = orc.gbm_paths(M, N, 100.0, R0, SIG0, T0, SEED, STREAM, off)
    return S, float(np.abs(S / So - 1).max()), 2e-5


def _heston(scheme):
    def run(ctx, M, off):
        S = host(ctx.heston_paths(M, N, 100.0, R0, T0, seed=SEED, stream=STREAM, pair_offset=off, scheme=scheme, **HP))
        So = orc.heston_paths(M, N, 100.0, R0, T0, seed=SEED, stream=STREAM, pair_offset=off, scheme=scheme, **HP)
        return S, float(np.abs(S / So - 1).max()), 5e-5
    return run


def _heston_qe(ctx, M, off):
    hp = qe.SET_B
    S = host(ctx.heston_paths(M, N, qe.MARKET["S0"], qe.MARKET["r"], qe.MARKET["T"], seed=SEED, stream=STREAM, pair_offset=off,
                              scheme=3, **hp))
    z1, z2 = qe.pair_view(host(ctx.gbm_normals(M // 2, 2 * N, SEED, STREAM, off)))
    ref = qe.paths(z1, z2, qe.MARKET["S0"], hp["v0"], qe.MARKET["r"], qe.MARKET["T"], hp["kappa"], hp["theta"], hp["xi"], hp["rho"])
    got = qe.compare(S, ref, qe.RTOL)  # asserts the bound on every column without a flagged step
    return S, got["worst"], qe.RTOL, ref["flagged"].any(axis=0)


GENERATORS = {"gbm": _gbm, "heston0": _heston(0), "heston1": _heston(1), "heston2": _heston(2), "heston3": _heston_qe}


@pytest.mark.parametrize("name", list(GENERATORS))
def test_every_generator_through_an_extreme_normal(ctx, name):
    run = GENERATORS[name]
    worst, cols, left_out = 0.0, 0, 0
    for r in re_.rows_of(FX, "tail", "radius"):
        for off, n_pairs, lane in placements(r["pair"]):
            S, dev, tol, *flag = run(ctx, 2 * n_pairs, off)
            assert S.shape == (N + 1, 2 * n_pairs) and np.isfinite(S).all(), (name, r, off)
            assert dev <= tol, (name, r, off, dev)
            worst = max(worst, dev)
            cols += 2
            if flag:
                left_out += int(flag[0][lane]) + int(flag[0][lane + n_pairs])
    note(f"generator {name}: worst deviation {worst:.3e} (bound {tol:.0e}); mined columns {cols}, left out by a discontinuity band {left_out}")
    assert left_out <= qe.MAX_SHARE * cols, (left_out, cols)  # the share tests/test_gpu_heston_qe.py allows


# ------------------------------------------------------------------ d. jump counts at equality and at their largest
@pytest.mark.parametrize("model,scheme", [("gbm", 0), ("heston", 0)])
@pytest.mark.parametrize("cls", ["count_edge", "count_max"])
def test_jump_counts_at_a_threshold_and_at_their_largest(ctx, cls, model, scheme):
    thr_fx = FX["jump_law"]["thr"]
    jump = (re_.JUMP_LAM, MU, SJ)
    worst = 0.0
    for i, r in enumerate(re_.rows_of(FX, cls)):
        for n_pairs, lane in ((4, i % 4), (1, 0)):
            M, off, t = 2 * n_pairs, r["pair"] - lane, r["step"]
            p = div_params(model, scheme, M=M, N=N, seed=SEED, stream=STREAM, pair_offset=off)
            thr, kappa, rj = _ffi.jump_table(p, jump, Q)
            assert [int(x) for x in thr] == thr_fx
            out, S = priced(ctx, p, jump, Q)
            assert np.isfinite(S).all() and (out["kappa"], out["drift_rate"]) == (kappa, rj)
            V = vanilla_at(ctx, p, rj)
            n, z = jr.draws(orc.philox4x32_10, n_pairs, N, SEED, STREAM, off, thr)
            assert n[t, lane] == r["count"], (r, n[:, lane])
            ref = jr.apply(V, n, z, MU, SJ)
            ok, w = dr.close(S, ref, ref, RTOL[model])
            worst = max(worst, w)
            assert ok, (model, r, M, w)
            first = jr.first_jump_step(n)
            before = np.arange(N + 1)[:, None] < np.concatenate([first, first])[None, :]
            assert np.array_equal(bits(S)[before], bits(V)[before]), (model, r, M)
            if cls == "count_edge" and r["k"] == 0:
                # directly: w == thr[0] is one jump at this step, w == thr[0] - 1 is none
                J = MU + SJ * z[t, lane]
                for col in (lane, lane + n_pairs):
                    growth = math.log((float(S[t, col]) / float(S[t - 1, col])) / (float(V[t, col]) / float(V[t - 1, col])))
                    if r["word"] == thr_fx[0]:
                        assert r["count"] == 1 and abs(J) > 1e-3 and abs(growth - J) <= 1e-5, (r, col, growth, J)
                        assert first[lane] <= t and S[t, col] != V[t, col]
                    else:
                        assert r["count"] == 0 and abs(growth) <= 1e-5, (r, col, growth)
                        if first[lane] > t:
                            assert np.array_equal(bits(S[:t + 1, col]), bits(V[:t + 1, col]))
    note(f"jumps {cls} {model}: worst error / bound {worst:.3f}")


# ------------------------------------------------------------------ e. bridge uniforms
def test_bridge_uniforms_of_zero_and_of_one_minus_an_ulp(ctx):
    assert (BS0, BR, BSIG, BT) == (re_.S0, re_.R, re_.SIG, re_.T) and (_H("down-and-out"), _H("up-and-out")) == re_.BARRIERS
    checked = 0
    for i, r in enumerate(re_.rows_of(FX, "bridge")):
        for n_pairs, lane in ((4, i % 4), (1, 0)):
            M, off, t = 2 * n_pairs, r["pair"] - lane, r["step"]
            p = barrier_params(M=M, N=N, seed=SEED, stream=STREAM, pair_offset=off)
            V = _vanilla(ctx, p)
            Z = orc.gbm_normals(n_pairs, N, SEED, STREAM, off)
            u = br.bridge_uniforms(n_pairs, N, SEED, STREAM, off)
            assert int(round(float(u[t - 1, lane]) * 2 ** 24)) == r["word"]
            for kind in br.KINDS:
                H = _H(kind)
                _, S = _barrier(ctx, p, kind, H, monitoring="continuous")
                hs, _ = br.continuous_hit_steps(V, Z, u, BS0, H, BR, BSIG, BT, kind)
                ref = br.encode(V, kind, H, hit_steps=hs, K=BK, is_put=True)
                for Hc, c in r["columns"]:
                    if Hc != H:
                        continue
                    col = lane + c * n_pairs
                    assert hs[col] == t if r["word"] != re_.W24 else hs[col] > t, (r, kind, col, hs)
                    assert np.array_equal(bits(S[:, col]), bits(ref[:, col])), (r, kind, M, col)  # no tie excuse here
                    checked += 1
    note(f"bridge: {checked} (row, kind, size, column) comparisons, all bit for bit")
    assert checked >= 4 * len(re_.rows_of(FX, "bridge"))  # two kinds per barrier, two sizes


# ------------------------------------------------------------------ the figures of DESIGN.md section 4
def test_report_the_measured_figures():
    """profiles/rng_edges.txt is this report: written where OMC_RNG_EDGES_REPORT points, printed otherwise"""
    assert sum(line.startswith("normals, class") for line in REPORT) == 3, "runs after the tests above"
    path = os.environ.get("OMC_RNG_EDGES_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("# tests/test_gpu_rng_edges.py on one MI355X (OMC_RNG_EDGES_REPORT=<this file> python -m pytest "
                    "tests/test_gpu_rng_edges.py -m gpu)\n# seed 0x%X stream 0x%X, fixture tests/golden/rng_edges.json\n" % (SEED, STREAM))
            f.write("\n".join(REPORT) + "\n")
