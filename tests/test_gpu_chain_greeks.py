"""The Greeks of a whole option chain, Bermudan entries included (omc_price_american_chain_greeks, include/omc_chain_greeks.h,
DESIGN.md section 35), held to the header's contract:

  1. an American entry equals its own omc_price_american_greeks call BIT FOR BIT -- every field of base but the times, every
     Greek and standard error, price_up / _down, n_exercised_up / _down, the policy -- whatever else the chain holds, in
     whatever order, at any "chain_greeks_k", on both storages;
  2. a Bermudan entry's policy is omc_price_american_chain's betas_out for it, bit for bit, and its result equals, bit for
     bit, the single call with that masked policy GIVEN (but base.sum_nitm, here the scheduled dates' sum); independently it
     agrees with the numpy restatement of the view's route (helpers/chain_greeks_ref.py) on the device's own matrix, and its
     counts and price with that chain's res[i];
  3. identical calls, duplicated entries and a reversed chain return identical bits;
  4. Heston entries have NaN vega, rho, theta.

Sizes: 4096 paths and 4098 on both storages ("fold_antithetic" forced on and off; 4098 folded = 2049 stored columns, the
one-column kernels); N in 1, 2 (no fit), 7, 13, 70 (walk_rows' batches of 8 with a ragged tail); k in 2, 3, 5, N-1, N, N+3;
GBM and Heston schemes 0, 1, 3; puts and calls; bump 0.01 and 0.5."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import chain_greeks_ref as cg
from helpers.chain_greeks_case import device_matrix, restate
from helpers.chain_greeks_case import same as _same
from helpers import greeks_check as gk
from options_model_amd import _ffi
from options_model_amd.pricer import BlackScholesGreeks as BSG

pytestmark = pytest.mark.gpu

C = _ffi.C
HESTON = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
@pytest.fixture
def cctx(ctx):
    yield ctx
    ctx.set_option("chain_greeks_k", -1)
    ctx.set_option("chain_greeks_order", 0)
    ctx.set_option("fold_antithetic", 1)


def _params(M, N, K=100.0, put=True, **kw):
    kw.setdefault("semantics", "two_pass")
    kw.setdefault("seed", 2025)
    kw.setdefault("stream", 4)
    kw.setdefault("pair_offset", 555)
    return _ffi.make_params(n_paths=M, n_steps=N, K=K, is_put=put, **kw)


def mixed_chain(N):
    """19 entries -- the second group of 16 holds three: both sides, a duplicated quote far from its twin, every schedule"""
    strikes = [90.0, 100.0, 105.0, 100.0, 97.0, 110.0, 100.0, 95.0, 103.0, 100.0, 92.0, 100.0, 108.0, 99.0, 101.0, 100.0,
               100.0, 96.0, 100.0]
    puts = [True, True, False, True, False, True, False, True, False, True, True, True, False, True, False, True,
            False, True, True]
    every = [0, 3, 0, 0, 5, N - 1, 2, 1, 0, 3, N, 0, 2, 0, 5, 1, N + 3, 0, N + 3]
    every = [max(k, 0) for k in every]
    assert len(strikes) == len(puts) == len(every) == 19
    return strikes, puts, every


def check_chain(c, M, N, folded, h, width, reverse, **kw):
    """The mixed chain against the contract, entry by entry.  -> the entries"""
    c.set_option("fold_antithetic", 2 if folded else 0)
    c.set_option("chain_greeks_k", width)
    strikes, puts, every = mixed_chain(N)
    if reverse:
        strikes, puts, every = strikes[::-1], puts[::-1], every[::-1]
    p = _params(M, N, **kw)
    outs, info = c.price_american_chain_greeks(p, strikes, puts, bump=h, want_betas=True, exercise_every=every)
    assert info["folded"] == int(folded) and info["n_groups"] == 2
    assert info["entries_per_launch"] == (16 if width < 1 else width)
    sides = [sum(puts[:16]), 16 - sum(puts[:16]), sum(puts[16:]), 3 - sum(puts[16:])]
    w = 16 if width < 1 else width
    assert info["n_sweep_launches"] == sum((s + w - 1) // w for s in sides)
    prices, _ = c.price_american_chain(p, strikes, puts, want_betas=True, exercise_every=every)
    S = device_matrix(c, p, folded)
    for i, (o, K, put, k) in enumerate(zip(outs, strikes, puts, every)):
        what = (M, N, folded, i, K, put, k)
        q = _params(M, N, K, put, **kw)
        assert o["n_paths"] == M and o["folded"] == int(folded) and o["bump"] == h
        assert np.array_equal(o["betas"], prices[i]["betas"]), what          # the chain's fits, bit for bit
        if k < 2:       # contract 1
            _same(o, c.price_american_greeks(q, bump=h, want_betas=True), what)
        else:           # contract 2
            one = c.price_american_greeks(q, bump=h, betas=o["betas"], want_betas=True)
            _same(o, one, what, skip=("sum_nitm",))
            assert one["sum_nitm"] == 0 and o["sum_nitm"] == int(o["betas"][1:N, 3].sum()), what
            assert not o["betas"][0].any() and not o["betas"][N].any()
            if k >= N:
                assert not o["betas"].any() and o["n_exercised"] == o["n_exercised_up"] == o["n_exercised_down"] == 0, what
        # the base against the chain's own pricing of the entry
        for key in ("n_exercised", "n_zero", "sum_nitm", "n_paths"):
            assert o[key] == prices[i][key], (what, key)
        assert abs(o["price"] - prices[i]["price"]) <= 1e-12 * max(1.0, abs(prices[i]["price"])), what
        # and, independently, the restatement of the view's route on the device's matrix
        gk.agrees(o, restate(S, p, K, put, k, o["betas"], h, folded), q)
        if p.model == 1:    # contract 4
            assert all(math.isnan(o[x]) and math.isnan(o["se_" + x]) for x in ("vega", "rho", "theta")), what
    return outs, (strikes, puts, every)


GBM_SHAPES = [(M, N, fold) for N in (1, 2, 7, 13, 70) for M in (4096, 4098) for fold in (True, False)]


@pytest.mark.parametrize("M,N,folded", GBM_SHAPES)
def test_gbm_chain_holds_the_contract(cctx, M, N, folded):
    i = GBM_SHAPES.index((M, N, folded))
    check_chain(cctx, M, N, folded, h=(0.01, 0.5)[(i + i // 2) % 2], width=(-1, 1, 3)[i % 3], reverse=bool((i + i // 4) % 2))


HESTON_SHAPES = [(M, N, (0, 1, 3)[(i + j) % 3]) for i, N in enumerate((1, 2, 7, 13, 70)) for j, M in enumerate((4096, 4098))]


@pytest.mark.parametrize("M,N,scheme", HESTON_SHAPES)
def test_heston_chain_holds_the_contract(cctx, M, N, scheme):
    i = HESTON_SHAPES.index((M, N, scheme))
    kw = dict(HESTON, model="heston", heston_scheme=scheme)
    if scheme == 3:
        kw.update(xi=0.6)       # the quadratic-exponential rule's exponential branch too
    check_chain(cctx, M, N, False, h=(0.5, 0.01)[i % 2], width=(3, -1, 1)[i % 3], reverse=bool(i % 2), **kw)


@pytest.mark.parametrize("folded", [True, False], ids=["folded", "full"])
def test_an_entry_alone_a_duplicate_a_reversed_chain_and_a_repeated_call(cctx, folded):
    """contract 3, and contract 1 at every "chain_greeks_k" and block order on ONE chain"""
    M, N, h = 4098, 13, 0.01
    ref, (strikes, puts, every) = check_chain(cctx, M, N, folded, h, -1, False)
    p = _params(M, N)
    _same(ref[1], ref[9], "duplicate")                       # (100 put every 3) twice, ten entries apart
    _same(ref[3], ref[11], "duplicate american")
    for width, order in ((-1, 0), (-1, 1), (1, 0), (3, 1), (16, 0)):
        cctx.set_option("chain_greeks_k", width)
        cctx.set_option("chain_greeks_order", order)
        for rev in (False, True):
            sl = slice(None, None, -1) if rev else slice(None)
            outs, _ = cctx.price_american_chain_greeks(p, strikes[sl], puts[sl], bump=h, want_betas=True, exercise_every=every[sl])
            for o, r in zip(outs, ref[sl]):
                _same(o, r, (width, order, rev))
    cctx.set_option("chain_greeks_k", -1)
    cctx.set_option("chain_greeks_order", 0)
    for i in (0, 1, 2, 5, 10, 16):                           # alone in its chain
        one, info = cctx.price_american_chain_greeks(p, [strikes[i]], [puts[i]], bump=h, want_betas=True, exercise_every=[every[i]])
        _same(one[0], ref[i], ("alone", i))
        assert info["n_groups"] == 1 and info["n_sweep_launches"] == 1


@pytest.mark.parametrize("folded", [True, False], ids=["folded", "full"])
def test_given_policies_with_holes(cctx, folded):
    """`betas`: one given policy per entry, n = 0 at some dates; pass 1 is skipped (sum_nitm = 0) for every entry"""
    M, N, h = 4096, 13, 0.5
    cctx.set_option("fold_antithetic", 2 if folded else 0)
    strikes, puts, every = [100.0, 95.0, 100.0, 104.0, 100.0], [True, True, False, False, True], [0, 0, 3, 1, N]
    p = _params(M, N)
    fitted, _ = cctx.price_american_chain_greeks(p, strikes, puts, bump=h, want_betas=True)
    given = np.stack([o["betas"] for o in fitted])
    given[:, 4] = 0.0
    given[1, 7:10, 3] = 0.0
    given[3, 1:N] = (5.0, -0.3, 0.01, 123.0)
    outs, _ = cctx.price_american_chain_greeks(p, strikes, puts, bump=h, betas=given, want_betas=True, exercise_every=every)
    S = device_matrix(cctx, p, folded)
    for i, (o, K, put, k) in enumerate(zip(outs, strikes, puts, every)):
        q = _params(M, N, K, put)
        used = cg.masked(given[i], k) if k >= 2 else given[i]
        assert np.array_equal(o["betas"], used) and o["sum_nitm"] == 0, i
        _same(o, cctx.price_american_greeks(q, bump=h, betas=used, want_betas=True), ("given", i))
        gk.agrees(o, restate(S, p, K, put, k, given[i], h, folded), q)
    assert outs[4]["n_exercised"] == 0 and outs[0]["n_exercised"] > 0


def test_no_early_date_is_black_scholes(cctx):
    """k >= N, fitted, and the all-zero given table on American entries: the same bits, and -- valued at t = dt -- e^{r dt}
    times Black-Scholes and its derivatives within 4 standard errors (the recipe of tests/test_gpu_greeks.py)"""
    S0, K, r, sig, T, N, M, h = 100.0, 100.0, 0.05, 0.2, 1.0, 50, 1_000_000, 0.01
    p = _params(M, N, seed=7, stream=1, pair_offset=0)
    a, _ = cctx.price_american_chain_greeks(p, [K, K], [True, False], bump=h, exercise_every=[N, N + 3])
    b, _ = cctx.price_american_chain_greeks(p, [K, K], [True, False], bump=h, betas=np.zeros((2, N + 1, 4)))
    dt = T / N
    e = math.exp(r * dt)
    for d, z, is_put in zip(a, b, (True, False)):
        _same(d, z, ("european", is_put))
        assert d["n_exercised"] == d["n_exercised_up"] == d["n_exercised_down"] == 0 and d["sum_nitm"] == 0
        kind = "put" if is_put else "call"
        bs = BSG.greeks(S0, K, T, r, sig, kind)
        C_ = BSG.black_scholes_price(S0, K, T, r, sig, kind)
        want = dict(delta=e * bs["Delta"], gamma=e * bs["Gamma"], vega=e * bs["Vega"] * 100,
                    rho=e * (dt * C_ + bs["Rho"] * 100), theta=e * (bs["Theta"] * 365 - r / N * C_))
        for k, v in want.items():
            slack = 2e-3 * abs(v) if k == "gamma" else 0.0  # the central difference's O(h^2)
            print(kind, k, d[k], v, d["se_" + k])
            assert abs(d[k] - v) <= 4 * d["se_" + k] + slack, (k, d[k], v, d["se_" + k])
        assert abs(d["price"] - e * C_) <= 4 * math.sqrt(max(d["sumsq"] / M - d["price"] ** 2, 0) / M)


def test_every_refusal_leaves_out_untouched(cctx):
    lib = cctx.lib
    good = _params(4096, 12)
    ent = (_ffi.ChainEntry * 3)()
    for x in ent:
        x.K, x.is_put, x.exercise_every = 100.0, 1, 3
    out = (_ffi.Greeks * 3)()
    raw = (C.c_char * C.sizeof(out)).from_buffer(out)
    raw[:] = b"\xa5" * len(raw)
    before = bytes(raw)

    def code(p=good, e=ent, n=3, bump=0.01, o=out):
        return lib.omc_price_american_chain_greeks(cctx.handle, C.byref(p) if p is not None else None, e, n, C.c_double(bump),
                                                   None, None, o, None)

    assert code(e=None) == -7 and bytes(raw) == before
    assert code(p=None) == -7 and bytes(raw) == before
    assert code(n=0) == -3 and code(n=257) == -3 and bytes(raw) == before
    bad = _params(4096, 12)
    bad.semantics = 0
    assert code(p=bad) == -4 and bytes(raw) == before
    bad = _params(4096, 12)
    bad.antithetic = 0
    assert code(p=bad) == -15 and bytes(raw) == before
    bad = _params(4096, 12)
    bad.n_steps = 0
    assert code(p=bad) != 0 and bytes(raw) == before             # omc_price_american's own refusal
    ent[1].K = 0.0
    assert code() == -4 and bytes(raw) == before
    ent[2].exercise_every = -1                                   # the entries' -4 comes before the schedule's -37
    assert code() == -4 and bytes(raw) == before
    ent[1].K = 100.0
    assert code() == -37 and b"exercise_every" in lib.omc_last_error() and bytes(raw) == before
    assert code(bump=0.0) == -37                                 # the chain's checks come before the bump's
    ent[2].exercise_every = 3
    ent[0].is_put = 2
    assert code() == -4 and bytes(raw) == before
    ent[0].is_put = 1
    for h in (0.0, -0.1, 0.6, float("nan")):
        assert code(bump=h) == -4 and b"bump" in lib.omc_last_error() and bytes(raw) == before
    assert code(o=None) == -7 and bytes(raw) == before
    assert code(bump=0.0, o=None) == -4                          # the bump's comes before the null out's
    # a distributed context (an all-reduce hook, as tests/test_gpu_chain.py installs one): refused after the entries' checks
    d = _ffi.Context(0)
    try:
        calls = []
        d.set_allreduce_hook(lambda dptr, count: calls.append(count))

        def dcode(bump=0.01):
            return lib.omc_price_american_chain_greeks(d.handle, C.byref(good), ent, 3, C.c_double(bump), None, None, out, None)

        assert dcode() == -10 and dcode(bump=0.0) == -10 and bytes(raw) == before
        ent[2].exercise_every = -1
        assert dcode() == -37 and bytes(raw) == before            # (-37 comes before -10, as in the chain)
        ent[2].exercise_every = 3
        d.set_allreduce_hook(None)
        assert calls == []
    finally:
        d.close()
    for v in (0, 17, -2):
        with pytest.raises(ValueError, match="chain_greeks_k"):
            cctx.set_option("chain_greeks_k", v)
    with pytest.raises(ValueError, match="exercise_every"):
        cctx.price_american_chain_greeks(good, [100.0], True, exercise_every=-2)
    assert code() == 0 and bytes(raw) != before
    assert out[0].base.n_paths == 4096 and out[0].delta < 0.0


def test_facades_against_the_context_call(cctx):
    from options_model_amd import exercise_dates, price_american_chain_greeks, price_american_greeks, price_bermudan_greeks
    args = dict(r=0.05, sigma=0.2, T=1.0, n_paths=8192, n_steps=24, seed=5)
    strikes, types, every = [95.0, 100.0, 100.0, 100.0, 104.0], ["put", "put", "put", "put", "call"], [0, 0, 6, 24, 2]
    chain = price_american_chain_greeks(100.0, strikes, option_types=types, exercise_every=every, bump=0.02, ctx=cctx, **args)
    assert len(chain) == 5 and chain.strikes == strikes and chain.option_types == types and chain.exercise_every == every
    assert set(chain.timings_ms) == {"paths", "pass1", "greeks", "total"}
    assert set(chain.info) == {"folded", "n_groups", "n_sweep_launches", "entries_per_launch"} and chain.info["n_groups"] == 1
    p = _ffi.make_params(model="gbm", is_put=True, semantics="two_pass", antithetic=True, n_paths=8192, n_steps=24, S0=100.0,
                         K=95.0, r=0.05, sigma=0.2, T=1.0, seed=5, stream=0)
    outs, info = cctx.price_american_chain_greeks(p, strikes, [t == "put" for t in types], bump=0.02, exercise_every=every)
    for e, ei, o, K, t, k in zip(chain.entries, chain.entry_info, outs, strikes, types, every):
        for f in ("price", "delta", "gamma", "vega", "rho", "theta", "se_delta", "se_gamma", "se_vega", "se_rho", "se_theta",
                  "price_up", "price_down", "bump", "n_paths", "n_exercised"):
            assert getattr(e, f) == o[f], (f, k)
        assert e.stderr == math.sqrt(max(o["sumsq"] / 8192 - o["price"] ** 2, 0.0) / 8192)
        assert e.folded == bool(info["folded"]) and e.model == "gbm" and e.option_type == t
        assert ei == dict(exercise_every=k, n_early_dates=len(exercise_dates(24, k)), sum_nitm=o["sum_nitm"])
        one = price_bermudan_greeks(100.0, K, exercise_every=k, option_type=t, bump=0.02,
                                    ctx=cctx, **args)
        for f in ("price", "stderr", "delta", "gamma", "vega", "rho", "theta", "se_delta", "price_up", "price_down", "n_exercised",
                  "folded", "model", "option_type"):
            assert getattr(one, f) == getattr(e, f), (f, k)
    am = price_american_greeks(100.0, 100.0, bump=0.02, ctx=cctx, **args)
    for f in ("price", "delta", "gamma", "vega", "rho", "theta", "se_gamma", "price_up", "n_exercised"):
        assert getattr(am, f) == getattr(chain.entries[1], f), f
    vals = [chain.entries[i] for i in (1, 2, 3)]                    # American, every 6th date, European: one strike
    assert vals[0].price > vals[1].price > vals[2].price > 0 and vals[2].n_exercised == 0
    h = price_bermudan_greeks(100.0, 100.0, exercise_every=6, model="Heston", heston_scheme="qe", ctx=cctx, **args)
    assert h.model == "heston" and math.isnan(h.vega) and math.isnan(h.se_theta) and h.delta < 0 and h.folded is False


def test_c_host_example_prints_the_entries(tmp_path, cctx):
    """examples/american_chain_greeks.c: a plain C host hedges a strike ladder on three schedules; the binding's values"""
    from options_model_amd import _build
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_chain_greeks"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_chain_greeks.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    out = subprocess.run([str(exe), "42", "100000"], check=True, capture_output=True, text=True, timeout=300).stdout
    rows = re.findall(r"^K\s+([0-9.]+) (\w+)\s+price ([0-9.]+)\s+delta (-?[0-9.]+)\s+gamma (-?[0-9.]+)\s+vega (-?[0-9.]+)\s+"
                      r"delta - european (-?[0-9.]+)\s+vega - european (-?[0-9.]+)", out, flags=re.M)
    assert [r[1] for r in rows] == ["american", "monthly", "european"] * 5 and "folded storage, 1 groups" in out
    strikes = [90.0 + 5.0 * (i // 3) for i in range(15)]
    assert [float(r[0]) for r in rows] == strikes
    outs, _ = cctx.price_american_chain_greeks(_params(100_000, 42, seed=42, stream=0, pair_offset=0), strikes, True, bump=0.01,
                                               exercise_every=[0, 21, 42] * 5)
    for i, (r, o) in enumerate(zip(rows, outs)):
        eu = outs[i // 3 * 3 + 2]
        for got, want in zip(r[2:], (o["price"], o["delta"], o["gamma"], o["vega"], o["delta"] - eu["delta"], o["vega"] - eu["vega"])):
            assert abs(float(got) - want) < 2e-6, (i, got, want)
    assert all(float(rows[3 * s + 2][6]) == 0.0 == float(rows[3 * s + 2][7]) for s in range(5))
