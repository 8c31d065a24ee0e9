"""Every kernel that takes the QE Heston step (heston_pair_step<3>) run with work to do.

tests/test_gpu_heston_qe.py ties the stored generator to the float64 restatement per spot; it runs the consumers only where
they do nothing (a barrier never touched, a dividend of 0, jumps of size 0).  Here they are live, and every comparison is with
the device's OWN ctx.heston_paths(..., scheme=3) matrix V on the same (seed, stream, pair_offset, rate): a consumer that
fused the shared step another way than the stored generator, took the other side of the branch ballot in a mixed wave or read
a stale constant misses V's bits.  No column is left out anywhere.  The laws are sets B (both branches in one wave) and C
(v0 = 0: every lane exponential at step 1), set A (quadratic only) besides for the register-only kernels; the cases and what
the restatement alone says of them are in tests/helpers/heston_qe_cases.py and tests/test_heston_qe_consumers_cpu.py.

What is compared, and how tightly -- every bound is the project's own, from the file named:
  * barrier           the kept matrix = barrier_ref.encode(V) bit for bit, hit_prob exact (test_gpu_barrier.py); the five
                      European fields of both styles under european_ref.sums_close / se_close (test_gpu_european_sums.py);
                      the American price against the C oracle's flow on the encoded device matrix: counts equal, 1e-9;
                      two pair_offset shards = the whole run bit for bit
  * dividends         dividend_ref.apply(V at r - q): rel 5e-5 of the column's largest vanilla spot, the rows before the
                      first dividend V's bits; the price: the oracle's flow on the device's matrix (test_gpu_dividends.py)
  * jumps             jump_ref.apply(V at rj): 5e-5, every column V's bits before its first jump; the price likewise
  * European sums     omc_price_european, its batch, omc_heston_price_strikes / _surface against V's last row under
                      sums_close / se_close; the batch = its single calls, the surface = its per-expiry calls, bit for bit
  * American paths    batch = single calls (counts, price 1e-12); chain and sequence = single calls bit for bit; the Greeks
                      against greeks_ref on V (helpers.greeks_check.agrees)
  * omc_heston_paths_from_normals_f32   refuses rho outside [-1, 1] and scheme 3 with v0 < 0 with -5, writing nothing
"""
import math

import numpy as np
import pytest

import test_gpu_barrier as gb
import test_gpu_chain as gc
import test_gpu_dividends as gd
import test_gpu_european_sums as es
import test_gpu_jumps as gj
import test_gpu_seq_group as gs
from helpers import barrier_ref as br
from helpers import dividend_ref as dr
from helpers import heston_qe_cases as qc
from helpers import heston_qe_ref as qe
from helpers import jump_ref as jr
from options_model_amd import _ffi

pytestmark = pytest.mark.gpu

QE = qc.QE
BOTH = ("B", "C")
bits = gd.bits


def kinds_at(levels):
    """(kind, H) of the four barrier kinds at a (down, up) pair"""
    return [(kind, levels[0] if kind.startswith("down") else levels[1]) for kind in br.KINDS]


def barrier_params(c, is_put=True, M=None, off=None):
    return gb._params("heston", QE, is_put=is_put, M=M or c["M"], N=c["N"], seed=c["seed"], stream=c["stream"],
                      pair_offset=c["off"] if off is None else off, **qc.LAWS[c["law"]])


# ---------------------------------------------------------------------------------------------- a. barrier, live
@pytest.mark.parametrize("name", list(qc.BARRIER_ENCODE))
def test_encoded_matrix_is_the_vanilla_matrix_encoded_bit_for_bit(ctx, name):
    c = qc.BARRIER_ENCODE[name]
    N = c["N"]
    for is_put in (True, False):
        p = barrier_params(c, is_put)
        V = gb._vanilla(ctx, p)
        dead = br.dead_spot(gb.K, is_put)
        for levels in qc.level_sets(c):
            for kind, H in kinds_at(levels):
                out, S = gb._barrier(ctx, p, kind, H)
                ref = br.encode(V, kind, H, K=gb.K, is_put=is_put)
                assert np.array_equal(bits(S), bits(ref)), (name, is_put, kind, H)
                hs = br.discrete_hit_steps(V, kind, H)
                t = np.arange(N + 1)[:, None]
                live = (t >= hs[None, :]) if kind.endswith("-in") else (t < hs[None, :])
                assert np.array_equal(bits(S[live]), bits(V[live]))
                assert np.all(bits(S[~live]) == bits(np.float32(dead)))
                assert 0 < (hs <= N).sum() < hs.size, (name, kind, H)  # the barrier is met by some paths, not all
                assert out["hit_prob"] == (hs <= N).mean()


@pytest.mark.parametrize("name", list(qc.BARRIER_EURO))
def test_barrier_sums_against_the_restatement(ctx, name):
    """barrier_paths_body + barrier_finalize_kernel at scheme 3: all five European fields of both styles"""
    c = qc.BARRIER_EURO[name]
    assert (c["seed"], c["off"]) == (es.SEED, es.OFFSET)
    for levels in qc.level_sets(c):
        seen = es._barrier_shape(ctx, "heston", QE, "discrete", c["M"], c["N"], stream=c["stream"], law=qc.LAWS[c["law"]],
                                 levels=levels)
        assert all(0 < h < c["M"] for h in seen), (name, levels, seen)  # both columns are fed


@pytest.mark.parametrize("name", list(qc.BARRIER_AMERICAN))
def test_american_barrier_matches_the_oracle_on_the_encoded_matrix(ctx, name):
    c = qc.BARRIER_AMERICAN[name]
    for is_put in (True, False):
        p = barrier_params(c, is_put)
        for levels in qc.level_sets(c):
            for kind, H in kinds_at(levels):
                out = gb._check_american(ctx, p, kind, H)
                assert 0.0 < out["hit_prob"] < 1.0


@pytest.mark.parametrize("name", list(qc.BARRIER_SHARD))
def test_two_pair_offset_shards_are_the_whole_barrier_run(ctx, name):
    c = qc.BARRIER_SHARD[name]
    M = c["M"]
    P, Ps = M // 2, M // 4
    for levels in qc.level_sets(c):
        for kind, H in kinds_at(levels)[1:3]:  # up-and-out, down-and-in
            _, whole = gb._barrier(ctx, barrier_params(c), kind, H)
            assert not np.array_equal(bits(whole), bits(gb._vanilla(ctx, barrier_params(c))))
            for k in range(2):
                _, sh = gb._barrier(ctx, barrier_params(c, M=M // 2, off=c["off"] + k * Ps), kind, H)
                assert np.array_equal(bits(sh[:, :Ps]), bits(whole[:, k * Ps:(k + 1) * Ps])), (name, kind, k)
                assert np.array_equal(bits(sh[:, Ps:]), bits(whole[:, P + k * Ps:P + (k + 1) * Ps])), (name, kind, k)


# ---------------------------------------------------------------------------------------------- b. dividends, live
@pytest.mark.parametrize("law", qc.DIV_LAWS)
@pytest.mark.parametrize("M,N", gd.SHAPES)
def test_dividend_matrix_matches_the_restatement_and_price_the_oracle(ctx, law, M, N):
    """dividend_ref.apply re-applies the vanilla matrix's own growth factors V_t / V_{t-1} to the spot that has paid its
    dividends.  The spot update of scheme 3 is multiplicative in s (s' = s exp(K0 + K1 v + K2 v' + sqrt(K3 v + K4 v') Zs), the
    variance never sees the spot), as the Euler schemes' is, so the restatement holds for it unchanged and at the same bound:
    rel 5e-5 of the column's largest vanilla spot for n_steps <= 64."""
    q = qc.div_yield(law)
    for is_put in (True, False):
        p = gd.params("heston", QE, is_put=is_put, M=M, N=N, seed=qc.DIV_SEED, stream=qc.DIV_STREAM, **qc.LAWS[law])
        divs, steps = gd.mixed_schedule(p, "heston")
        out, S = gd.priced(ctx, p, q, divs)
        V, has = gd.check_matrix(ctx, p, q, divs, S, "heston")
        assert list(np.nonzero(has)[0]) == steps and out["n_div_steps"] == len(steps) and out["first_div_step"] == steps[0]
        assert out["folded"] == 0 and out["n_paths"] == M
        assert not np.array_equal(bits(S[steps[0]]), bits(V[steps[0]]))  # the dividends are paid
        gd.check_price(out, S, p)


@pytest.mark.parametrize("law", qc.DIV_LAWS)
def test_a_cash_dividend_that_takes_paths_to_zero(ctx, law):
    z = qc.DIV_ZERO
    N = z["N"]
    for is_put in (True, False):
        p = gd.params("heston", QE, is_put=is_put, M=z["M"], N=N, seed=z["seed"], stream=z["stream"], **qc.LAWS[law])
        divs = gd.at_steps(p, [N // 2], [(z["cash"][law], "cash")])
        out, S = gd.priced(ctx, p, z["q"], divs)
        zero = S[N // 2] == 0.0
        print(f"set {law} put={is_put}: {100 * zero.mean():.2f} % of the columns at 0 from step {N // 2}")
        assert 0.01 <= zero.mean() <= 0.50
        assert np.all(S[N // 2:, zero] == 0.0) and np.all(S[:N // 2] > 0.0)
        gd.check_matrix(ctx, p, z["q"], divs, S, "heston")
        ref = gd.check_price(out, S, p)
        assert math.isfinite(out["price"]) and out["price"] > 0.0 and ref["n_exercised"] > 0


# ---------------------------------------------------------------------------------------------- c. jumps, live (Bates under QE)
@pytest.mark.parametrize("law", qc.JUMP_LAWS)
@pytest.mark.parametrize("M,N", gd.SHAPES[:4])
def test_jump_matrix_matches_the_restatement_and_price_the_oracle(ctx, law, M, N):
    lam = gj.lam_of(N)
    for is_put, stream, off in qc.JUMP_COORDS:
        p = gd.params("heston", QE, is_put=is_put, M=M, N=N, seed=qc.JUMP_SEED, stream=stream, pair_offset=off, **qc.LAWS[law])
        thr, kappa, rj = _ffi.jump_table(p, (lam, gj.MU, gj.SJ), gj.Q)
        out, S = gj.priced(ctx, p, (lam, gj.MU, gj.SJ), gj.Q)
        assert out["folded"] == 0 and out["n_paths"] == M and (out["kappa"], out["drift_rate"]) == (kappa, rj)
        assert out["n_thresholds"] == int((thr < (1 << 24)).sum())
        if is_put or M <= 5_000:  # (the restatement's Philox loop runs once per large shape)
            V = gj.vanilla_at(ctx, p, rj)
            n, z = gj.draws(M // 2, N, int(p.seed), int(p.stream), int(p.pair_offset), tuple(int(t) for t in thr))
            ref = jr.apply(V, n, z, gj.MU, gj.SJ)
            ok, worst = dr.close(S, ref, ref, gd.RTOL["heston"])
            print(f"set {law} {M}x{N} put={is_put}: worst error / bound {worst:.3f}, jump cells {(n > 0).mean():.4f}")
            assert ok, (law, M, N, worst)
            first = jr.first_jump_step(n)
            before = np.arange(N + 1)[:, None] < np.concatenate([first, first])[None, :]
            assert np.array_equal(bits(S)[before], bits(V)[before])
            assert (n[1:] > 0).any() and (n[1:] == 0).any() and not np.array_equal(bits(S), bits(V))
            if (M, N) == qc.BALLOT_SHAPE:
                # both sides of the kernel's wave ballot ("no lane of this wave jumps") are taken with exponential lanes in
                # them: from the counts and the restatement's branches at the drift rate rj
                expo = qc.restated(law, M, N, qc.JUMP_SEED, stream, off, rj)["expo"]
                jumps = np.concatenate([n[1:] > 0, n[1:] > 0], axis=1)
                wave_jumps, wave_expo = qc.wave_any(jumps, M), qc.wave_any(expo, M)
                assert (wave_jumps & wave_expo).any() and (~wave_jumps & wave_expo).any(), (law, stream)
        gd.check_price(out, S, p)


# ---------------------------------------------------------------------------------------------- e. register-only kernels
@pytest.mark.parametrize("law", list(qc.LAWS))
def test_price_european_sums_against_the_stored_last_row(ctx, law):
    L = qc.LAWS[law]
    for M, N in es._european_cases("heston", True):
        V = es._matrix(ctx, es._params("heston", QE, True, M, N, stream=qc.EURO_STREAM, law=L))
        for is_put in (True, False):
            p = es._params("heston", QE, is_put, M, N, stream=qc.EURO_STREAM, law=L)
            es._check_european(ctx.price_european(p), V[-1], is_put, (law, M, N, is_put))


@pytest.mark.parametrize("law", list(qc.LAWS))
def test_price_european_batch_sums_against_the_stored_last_row(ctx, law):
    L = qc.LAWS[law]
    ps = [es._params("heston", QE, i % 2 == 0, M, N, stream=4 + i, law=L) for i, (M, N) in enumerate(qc.EURO_BATCH)]
    out = ctx.price_european_batch(ps)
    assert len(out) == len(ps)
    for p, res in zip(ps, out):
        es._check_european(res, es._matrix(ctx, p)[-1], bool(p.is_put), (law, p.n_paths, p.n_steps))
        one = ctx.price_european(p)
        assert (res["sum"], res["sumsq"], res["n_zero"], res["std"]) == (one["sum"], one["sumsq"], one["n_zero"], one["std"])


@pytest.mark.parametrize("M", es.STRIKE_M)
@pytest.mark.parametrize("law", list(qc.LAWS))
def test_strike_prices_and_stderrs_against_the_stored_last_row(ctx, law, M):
    h = qc.LAWS[law]
    for N in es.STRIKE_N:
        row = es._row(ctx, M, N, es.T, QE, stream=qc.STRIKE_STREAM, law=h)
        for is_put in (True, False):
            for count in es.STRIKE_COUNTS:
                ks = es._strikes(row, is_put, count)
                prices, errs = ctx.heston_price_strikes(M, N, es.S0, es.R, es.T, h["v0"], h["kappa"], h["theta"], h["xi"],
                                                        h["rho"], ks, is_put=is_put, seed=es.SEED, stream=qc.STRIKE_STREAM,
                                                        scheme=QE)
                assert es._check_quotes(prices, errs, ks, row, math.exp(-es.R * es.T), is_put, (law, M, N, is_put, count))
                spot = ks[0 if count == 1 else (2 if count == 3 else 3)]
                assert es.er.sums(row, float(spot), 1.0, is_put, False)["n_zero"] >= 1  # the p > 0 edge is met


@pytest.mark.parametrize("law", list(qc.LAWS))
def test_surface_against_each_expiry_row_and_its_per_expiry_calls(ctx, law):
    h, M, N = qc.LAWS[law], es.SURFACE_M, qc.SURFACE["N"]
    a = (h["v0"], h["kappa"], h["theta"], h["xi"], h["rho"])
    expiries, streams = qc.SURFACE["expiries"], qc.SURFACE["streams"]
    rows = [es._row(ctx, M, N, Te, QE, stream=s, law=h) for Te, s in zip(expiries, streams)]
    rng = np.random.default_rng(5)
    for is_put in (True, False):
        ks = np.concatenate([es._strikes(r, is_put, 8) for r in rows])
        eo = np.repeat(np.arange(3), 8)
        order = rng.permutation(ks.size)
        ks, eo = ks[order], eo[order]
        prices, errs = ctx.heston_price_surface(M, N, es.S0, es.R, *a, expiries, streams, ks, eo, is_put=is_put, seed=es.SEED,
                                                scheme=QE)
        for e in range(3):
            sel = eo == e
            assert es._check_quotes(prices[sel], errs[sel], ks[sel], rows[e], math.exp(-es.R * expiries[e]), is_put,
                                    (law, "surface", e, is_put))
            one, one_err = ctx.heston_price_strikes(M, N, es.S0, es.R, float(expiries[e]), *a, ks[sel], is_put=is_put,
                                                    seed=es.SEED, stream=int(streams[e]), scheme=QE)
            assert np.array_equal(prices[sel], one) and np.array_equal(errs[sel], one_err), (law, e, is_put)


# ---------------------------------------------------------------------------------------------- f. American pricing paths
def american_params(law, M, N, is_put, stream, K=qc.K):
    return _ffi.make_params(model="heston", heston_scheme="qe", is_put=is_put, semantics="two_pass", n_paths=M, n_steps=N,
                            S0=qc.S0, K=K, r=qc.R, sigma=0.0, T=qc.T, seed=qc.AMERICAN_SEED, stream=stream, **qc.LAWS[law])


@pytest.mark.parametrize("law", BOTH)
def test_batched_pricings_are_the_single_calls(ctx, law):
    ps = [american_params(law, M, N, i % 2 == 0, 4 + i) for i, (M, N) in enumerate(qc.BATCH_SHAPES)]
    for p, res in zip(ps, ctx.price_american_batch(ps)):
        one = ctx.price_american(p)
        assert (res["n_exercised"], res["n_zero"], res["sum_nitm"]) == (one["n_exercised"], one["n_zero"], one["sum_nitm"])
        assert abs(res["price"] - one["price"]) <= 1e-12 * abs(one["price"]) and one["price"] > 0.0


@pytest.mark.parametrize("law", BOTH)
def test_chain_returns_every_entry_with_the_bits_of_its_single_call(ctx, law):
    c = qc.CHAIN
    kw = dict(model="heston", heston_scheme="qe", S0=qc.S0, r=qc.R, T=qc.T, seed=qc.AMERICAN_SEED, stream=6, **qc.LAWS[law])
    singles, fits = gc._singles(ctx, c["M"], c["N"], c["strikes"], c["puts"], **kw)
    assert len({s["price"] for s in singles}) == len(singles)
    assert all(s["n_exercised"] > 0 for s, put in zip(singles, c["puts"]) if put)  # (a call is not exercised early here)
    _, info = gc._check_chain(ctx, c["M"], c["N"], c["strikes"], c["puts"], singles, fits, law, **kw)
    assert info["fused"] == 0 and info["folded"] == 0
    gc._check_chain(ctx, c["M"], c["N"], c["strikes"][::-1], c["puts"][::-1], singles[::-1], fits[::-1], (law, "reversed"), **kw)


@pytest.mark.parametrize("law", BOTH)
def test_every_member_of_a_sequence_returns_its_own_bits(ctx, law):
    s = qc.SEQ
    ps = [american_params(law, s["M"], s["N"], i % 2 == 0, i) for i in range(s["n"])]
    singles = [ctx.price_american(p) for p in ps]
    outs = ctx.price_american_seq(ps)
    assert len(outs) == len(ps) and len({o["price"] for o in outs}) == len(ps)
    for p, o, one in zip(ps, outs, singles):
        gs._same(o, one)
        assert o["folded"] == 0 and (o["n_exercised"] > 0 or not p.is_put)


def test_greeks_where_every_lane_starts_exponential(ctx):
    from helpers import greeks_ref as gr
    from helpers.greeks_check import agrees

    g = qc.GREEKS
    h = qc.LAWS["C"]
    Vd = ctx.heston_paths(g["M"], g["N"], qc.S0, qc.R, qc.T, *qc.law_args("C"), g["seed"], g["stream"], 0, QE)
    V = Vd.to_host()
    Vd.free()
    for is_put in (True, False):
        p = _ffi.make_params(model="heston", heston_scheme=QE, is_put=is_put, semantics="two_pass", n_paths=g["M"],
                             n_steps=g["N"], S0=qc.S0, K=qc.K, r=qc.R, sigma=0.0, T=qc.T, seed=g["seed"], stream=g["stream"], **h)
        d = ctx.price_american_greeks(p, bump=0.01, want_betas=True)
        assert agrees(d, gr.greeks(V, qc.K, qc.R, qc.T, is_put, d["betas"], qc.S0, 0.0, h=0.01, gbm=False), p), is_put
        assert (d["n_exercised"] > 0 or not is_put) and (d["delta"] < 0.0) == is_put


# ---------------------------------------------------------------------------------------------- 4. the from-normals arguments
def test_from_normals_refuses_what_the_other_generators_refuse(ctx):
    M, N = 64, 4
    h = qc.LAWS["A"]
    z = ctx.to_device(np.full((N, M // 2), 0.25, np.float32))
    S = ctx.to_device(np.full((N + 1, M), 7.0, np.float32))
    V = ctx.to_device(np.full((N + 1, M), 7.0, np.float32))
    try:
        def rc(scheme, **over):
            a = dict(h, **over)
            return ctx.lib.omc_heston_paths_from_normals_f32(ctx.handle, S.ptr, M, M, N, qc.S0, qc.R, qc.T, a["v0"], a["kappa"],
                                                             a["theta"], a["xi"], a["rho"], z.ptr, z.ptr, M // 2, scheme)

        def rc_sv(scheme, **over):
            a = dict(h, **over)
            return ctx.lib.omc_heston_paths_sv_f32(ctx.handle, S.ptr, V.ptr, M, M, N, qc.S0, qc.R, qc.T, a["v0"], a["kappa"],
                                                   a["theta"], a["xi"], a["rho"], qe.SEED, 0, 0, scheme)

        for v0 in (-0.01, -1e-300, float("nan")):
            assert rc(QE, v0=v0) == -5 and rc_sv(QE, v0=v0) == -5, v0
        assert b"invalid Heston parameters" in ctx.lib.omc_last_error()
        for scheme in (0, 1, 2, QE):
            for rho in (1.0000001, -1.5, float("nan"), float("inf")):
                assert rc(scheme, rho=rho) == -5 and rc_sv(scheme, rho=rho) == -5, (scheme, rho)
        assert rc(QE, v0=float("nan"), rho=2.0) == -5
        assert np.all(S.to_host() == 7.0) and np.all(V.to_host() == 7.0)  # nothing was written
        with pytest.raises(ValueError, match="invalid Heston parameters"):
            ctx.heston_paths_from_normals(np.zeros((N, 2), np.float32), np.zeros((N, 2), np.float32), qc.S0, qc.R, qc.T,
                                          -0.01, h["kappa"], h["theta"], h["xi"], h["rho"], QE)
        # what stays: a stored full-truncation state is a start state, schemes 0 and 2 floor it, rho = +-1 is a correlation
        for scheme in (0, 1, 2):
            assert rc(scheme, v0=-0.01) == 0, scheme
        X = S.to_host()
        assert np.isfinite(X).all() and np.all(X[0] == np.float32(qc.S0)) and X.min() > 0.0
        assert rc(QE, v0=0.0) == 0 and rc(QE, rho=-1.0) == 0 and rc(1, rho=1.0) == 0
        assert np.isfinite(S.to_host()).all()
    finally:
        for a in (z, S, V):
            a.free()
    # the context still prices
    assert ctx.price_american(american_params("A", 4096, 8, True, 0))["price"] > 0.0
