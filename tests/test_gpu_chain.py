"""A whole American option chain from one set of paths (omc_price_american_chain, omc_chain_width).

One generator launch and one path matrix serve every strike and side of an expiry; on folded storage the fused sweeps read
every stored spot once for all entries of a launch.  THE CONTRACT: entry i of a chain returns the BITS of its own
omc_price_american call -- price, sums, counts, storage -- and the fits that call makes (omc_price_american_greeks returns
them: same pass 1, same solve), whatever else the chain holds, in whatever order, on either route, at any width."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("price", "sum", "sumsq", "std", "zero_prob", "n_exercised", "n_zero", "sum_nitm", "n_paths", "folded")
# puts with a duplicate, then calls: 7 entries
STRIKES = (80.0, 95.0, 100.0, 100.0, 110.0, 100.0, 105.0)
PUTS = (True, True, True, True, True, False, False)


def _same(a, b, what=""):
    for k in KEYS:
        assert a[k] == b[k], (what, k, a[k], b[k])


@pytest.fixture
def cctx(ctx):
    yield ctx
    ctx.set_option("chain_fused", 0)
    ctx.set_option("chain_k", -1)
    ctx.set_option("pass2_tables", 1)
    ctx.set_option("pass2_tables_irregular_every", 0)
    ctx.set_option("fold_antithetic", 1)


def _params(M, N, K=100.0, put=True, **kw):
    from options_model_amd import _ffi
    kw.setdefault("semantics", "two_pass")
    kw.setdefault("seed", 11)
    return _ffi.make_params(n_paths=M, n_steps=N, K=K, is_put=put, **kw)


def _singles(c, M, N, strikes, puts, fits=True, **kw):
    res = [c.price_american(_params(M, N, K, put, **kw)) for K, put in zip(strikes, puts)]
    bet = [c.price_american_greeks(_params(M, N, K, put, **kw), want_betas=True)["betas"] if fits else None
           for K, put in zip(strikes, puts)]
    return res, bet


def _check_chain(c, M, N, strikes, puts, singles, fits, what="", **kw):
    outs, info = c.price_american_chain(_params(M, N, 1.0, True, **kw), strikes, puts, want_betas=True)
    assert len(outs) == len(strikes)
    for i, (o, s, b) in enumerate(zip(outs, singles, fits)):
        _same(o, s, (what, i))
        if b is not None:
            assert np.array_equal(o["betas"], b), (what, i)
        assert o["timed"] == (1 if i == 0 else 0)
        assert o["ms_total"] == info["ms_total"] and o["ms_paths"] == info["ms_paths"]
    assert info["ms_total"] > 0 and info["ms_paths"] > 0
    return outs, info


@pytest.mark.parametrize("M,N,folded", [
    (65_536, 9, 1),         # the smallest folded pricing; one time chunk
    (200_000, 50, 1),       # ragged tiles
    (1_000_000, 252, 1),    # the headline geometry
    (4_000, 30, 0),         # full storage
])
def test_chain_returns_every_entry_with_the_bits_of_its_single_call(cctx, M, N, folded):
    singles, fits = _singles(cctx, M, N, STRIKES, PUTS)
    assert all(s["folded"] == folded for s in singles)
    _same(singles[2], singles[3])
    assert len({s["price"] for s in singles}) == len(STRIKES) - 1
    p = _params(M, N, 1.0, True)
    widths = {}
    for fused in (1, 0):
        cctx.set_option("chain_fused", fused)
        for k in (1, 2, 3, -1, 16):
            cctx.set_option("chain_k", k)
            widths[(fused, k)] = cctx.chain_width(p, len(STRIKES))
            outs, info = _check_chain(cctx, M, N, STRIKES, PUTS, singles, fits, (fused, k))
            assert info["folded"] == folded and info["fused"] == (fused if folded else 0)
            _same(outs[2], outs[3])                 # the duplicate: identical bits
            assert np.array_equal(outs[2]["betas"], outs[3]["betas"])
            # the reversed chain: the same per-entry bits
            _check_chain(cctx, M, N, STRIKES[::-1], PUTS[::-1], singles[::-1], fits[::-1], (fused, k, "reversed"))
    assert all(widths[(0, k)] == 1 for k in (1, 2, 3, -1, 16))
    if folded:
        assert widths[(1, 1)] == 1 and widths[(1, 2)] == 2 and widths[(1, 3)] == 2
        assert widths[(1, -1)] == widths[(1, 16)] == 4
    else:
        assert all(widths[(1, k)] == 1 for k in (1, 2, 3, -1, 16))


def test_four_columns_per_thread_from_4m_paths(cctx):
    """From 2^21 stored columns on the folded pass 2 takes four columns per thread: the chain's two-entry instantiations."""
    M, N = 8_388_608, 9
    strikes, puts = (95.0, 100.0, 104.0, 100.0, 105.0), (True, True, True, False, False)
    singles, fits = _singles(cctx, M, N, strikes, puts)
    assert cctx.chain_width(_params(M, N), len(strikes)) == 1      # the default route is the unfused one
    cctx.set_option("chain_fused", 1)
    assert cctx.chain_width(_params(M, N), len(strikes)) == 2
    for fused in (1, 0):
        cctx.set_option("chain_fused", fused)
        _, info = _check_chain(cctx, M, N, strikes, puts, singles, fits, ("8M", fused))
        assert info["fused"] == fused and info["folded"] == 1
        if fused:
            assert info["n_launch_groups"] == 3          # puts 2 + 1, calls 2


def test_nine_puts_on_scalar_loads(cctx):
    """Stored columns not a multiple of four: one column per thread; nine quotes of one side go as 4 + 4 + 1."""
    M, N = 100_002, 40
    strikes = [80.0 + 4.0 * i for i in range(9)]
    singles, fits = _singles(cctx, M, N, strikes, [True] * 9, sigma=0.3)
    for fused in (1, 0):
        cctx.set_option("chain_fused", fused)
        _, info = _check_chain(cctx, M, N, strikes, [True] * 9, singles, fits, ("vec1", fused), sigma=0.3)
        assert info["n_launch_groups"] == (3 if fused else 9)


def test_tables_beyond_32k_of_lds(cctx):
    """300 steps x 4 entries: 38.5 KB of exercise tables per workgroup, above what a kernel may take without asking."""
    M, N = 131_072, 300
    strikes, puts = (90.0, 100.0, 105.0, 110.0, 100.0), (True, True, True, True, False)
    singles, fits = _singles(cctx, M, N, strikes, puts)
    cctx.set_option("chain_fused", 1)
    assert cctx.chain_width(_params(M, N), len(strikes)) == 4
    _, info = _check_chain(cctx, M, N, strikes, puts, singles, fits, "N=300")
    assert info["fused"] == 1 and info["n_launch_groups"] == 2


def test_deep_out_of_the_money_put_never_exercises(cctx):
    M, N = 131_072, 30
    kw = dict(T=0.5)  # S0 = 100, sigma = 0.2: a spot below 40 is 6.6 standard deviations away
    single = cctx.price_american(_params(M, N, 40.0, True, **kw))
    assert single["n_exercised"] == 0 and single["sum_nitm"] == 0   # no step has a regression set
    for fused in (1, 0):
        cctx.set_option("chain_fused", fused)
        (o,), info = cctx.price_american_chain(_params(M, N, **kw), [40.0], True)
        _same(o, single)
        assert o["n_exercised"] == 0 and o["price"] == 0.0
        outs, _ = cctx.price_american_chain(_params(M, N, **kw), [100.0, 40.0, 95.0], True)
        _same(outs[1], single)
        _same(outs[0], cctx.price_american(_params(M, N, 100.0, True, **kw)))


@pytest.mark.parametrize("M,N", [(131_072, 30), (4_000, 30), (131_072, 1)])
def test_chain_of_one_equals_the_single_call(cctx, M, N):
    for K, put in ((100.0, True), (105.0, False)):
        single = cctx.price_american(_params(M, N, K, put))
        for fused in (1, 0):
            cctx.set_option("chain_fused", fused)
            (o,), info = cctx.price_american_chain(_params(M, N), [K], put)
            _same(o, single)


@pytest.mark.parametrize("M", [100_002, 200_000], ids=["vec1", "vec2"])
def test_forced_irregular_table_steps(cctx, M):
    N = 50
    base, fits = _singles(cctx, M, N, STRIKES, PUTS, sigma=0.4)
    cctx.set_option("pass2_tables_irregular_every", 3)
    singles, _ = _singles(cctx, M, N, STRIKES, PUTS, fits=False, sigma=0.4)
    for s, b in zip(singles, base):
        _same(s, b)                                 # the same decisions either way (test_gpu_pass2_tables.py)
    for fused in (1, 0):
        cctx.set_option("chain_fused", fused)
        _, info = _check_chain(cctx, M, N, STRIKES, PUTS, singles, fits, ("irregular", fused), sigma=0.4)
        assert info["fused"] == fused
    cctx.set_option("pass2_tables_irregular_every", 0)
    cctx.set_option("pass2_tables", 0)
    cctx.set_option("chain_fused", 1)
    singles, _ = _singles(cctx, M, N, STRIKES, PUTS, fits=False, sigma=0.4)
    _, info = _check_chain(cctx, M, N, STRIKES, PUTS, singles, fits, "no tables", sigma=0.4)
    assert info["fused"] == 0 and info["folded"] == 1   # the fused pass 2 decides from tables: without them, the single sweeps
    assert cctx.chain_width(_params(M, N, sigma=0.4), len(STRIKES)) == 1


def test_heston_chain_takes_the_unfused_route(cctx):
    M, N = 131_072, 30
    strikes, puts = (95.0, 100.0, 105.0), (True, False, True)
    kw = dict(model="heston", heston_scheme="full_truncation")
    cctx.set_option("chain_fused", 1)       # asked for or not
    singles, fits = _singles(cctx, M, N, strikes, puts, **kw)
    _, info = _check_chain(cctx, M, N, strikes, puts, singles, fits, "heston", **kw)
    assert info["fused"] == 0 and info["folded"] == 0


def test_more_entries_than_one_group(cctx):
    M, N = 65_536, 12
    strikes = [70.0 + 1.5 * i for i in range(37)]
    puts = [i % 3 != 0 for i in range(37)]
    singles, _ = _singles(cctx, M, N, strikes, puts, fits=False)
    for fused in (1, 0):
        cctx.set_option("chain_fused", fused)
        _check_chain(cctx, M, N, strikes, puts, singles, [None] * 37, ("groups", fused))


def test_stated_error_codes(cctx):
    from options_model_amd import _ffi
    lib = cctx.lib

    def call(c, p, strikes, puts=True):
        with pytest.raises(ValueError) as ei:   # (the binding raises ValueError for the library's argument errors)
            c.price_american_chain(p, strikes, puts)
        return str(ei.value)

    def code(c, p, entries, n):
        res = (_ffi.Result * max(n, 1))()
        return lib.omc_price_american_chain(c.handle, _ffi.C.byref(p), entries, n, res, None, None)

    ent = (_ffi.ChainEntry * 257)()
    for x in ent:
        x.K, x.is_put = 100.0, 1
    good = _params(131_072, 30)
    assert code(cctx, good, ent, 3) == 0
    assert code(cctx, good, ent, 0) == -3 and code(cctx, good, ent, 257) == -3
    assert code(cctx, good, None, 3) == -7
    assert lib.omc_price_american_chain(cctx.handle, _ffi.C.byref(good), ent, 3, None, None, None) == -7
    assert code(cctx, _params(131_072, 30, semantics="reference"), ent, 3) == -4
    assert code(cctx, _params(131_072, 30, antithetic=False), ent, 3) == -15
    ent[1].K = 0.0
    assert code(cctx, good, ent, 3) == -4
    ent[1].K = float("inf")
    assert code(cctx, good, ent, 3) == -4
    ent[1].K, ent[1].is_put = 100.0, 2
    assert code(cctx, good, ent, 3) == -4
    ent[1].is_put = 1
    assert "strike" in call(cctx, good, [100.0, 0.0])
    assert cctx.chain_width(good, 0) == 0 and cctx.chain_width(good, 257) == 0
    assert cctx.chain_width(_params(131_072, 30, semantics="reference"), 3) == 0
    # a distributed context (an all-reduce hook, as tests/test_gpu_seq_group.py installs one): refused, nothing launched
    c = _ffi.Context(0)
    try:
        calls = []
        c.set_allreduce_hook(lambda dptr, count: calls.append(count))
        assert code(c, good, ent, 3) == -10
        assert c.chain_width(good, 3) == 0
        c.set_allreduce_hook(None)
        assert calls == [] and code(c, good, ent, 3) == 0
    finally:
        c.close()


def test_facade_chain_equals_three_facade_calls(cctx):
    from options_model_amd import price_american_chain, price_american_option
    args = dict(r=0.05, sigma=0.2, T=1.0, n_paths=131_072, n_steps=30, seed=5)
    strikes, types = [90.0, 100.0, 110.0], ["put", "call", "put"]
    chain = price_american_chain(100.0, strikes, option_types=types, ctx=cctx, **args)
    assert chain.strikes == strikes and chain.option_types == types and len(chain.entries) == 3
    assert chain.info["folded"] is True and chain.info["fused"] is False and chain.timings_ms["total"] > 0
    cctx.set_option("chain_fused", 1)
    fused = price_american_chain(100.0, strikes, option_types=types, ctx=cctx, **args)
    assert fused.info["fused"] is True and [e.price for e in fused.entries] == [e.price for e in chain.entries]
    for e, K, ot in zip(chain.entries, strikes, types):
        one = price_american_option(100.0, K, option_type=ot, ctx=cctx, **args)
        for f in ("price", "stderr", "std", "zero_prob", "n_paths", "n_exercised", "sum_nitm", "model", "semantics",
                  "option_type"):
            assert getattr(e, f) == getattr(one, f), (K, f)
        assert set(e.timings_ms) == set(one.timings_ms)
    puts = price_american_chain(100.0, strikes, ctx=cctx, **args)          # one side for all
    assert puts.entries[0].price == chain.entries[0].price and puts.option_types == ["put"] * 3
    heston = price_american_chain(100.0, [100.0], model="Heston", ctx=cctx, **args)
    assert heston.info["fused"] is False and heston.entries[0].price == price_american_option(
        100.0, 100.0, model="Heston", ctx=cctx, **args).price


def test_c_host_example_prints_the_chain(tmp_path, cctx):
    """examples/american_chain.c: a plain C host prices ten quotes through the ABI; the prices the binding's singles give."""
    import os
    import re
    import shutil
    import subprocess

    from options_model_amd import _build
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_chain"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_chain.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    out = subprocess.run([str(exe), "50", "200000"], check=True, capture_output=True, text=True, timeout=300).stdout
    rows = re.findall(r"^(put|call)\s+K =\s*([0-9.]+)\s+price ([0-9.]+)", out, flags=re.M)
    assert len(rows) == 10 and "folded storage, single-strike sweeps" in out
    for side, K, price in rows:
        one = cctx.price_american(_params(200_000, 50, float(K), side == "put", seed=42))
        assert abs(float(price) - one["price"]) < 1e-6, (side, K)
