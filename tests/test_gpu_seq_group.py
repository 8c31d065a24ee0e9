"""Two-pass sequences in groups (omc_price_american_seq, option "seq_two_pass_k"; omc_seq_group_width).

A run of two-pass pricings of one geometry on folded storage shares its latency-bound launches: the pass-1 reductions,
the table builds and the finalizes of K pricings run as three launches with the pricing on the grid, around the bodies
of the single launches.  The contract is that of the per-step flows (test_gpu_step_multi.py): every pricing of the
sequence returns the BITS of its own omc_price_american call, whatever K, and whatever else the sequence holds."""
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("price", "sum", "sumsq", "n_exercised", "n_zero", "sum_nitm", "n_paths", "folded")


def _same(a, b):
    for k in KEYS:
        assert a[k] == b[k], (k, a[k], b[k])


@pytest.fixture
def gctx(ctx):
    yield ctx
    ctx.set_option("seq_two_pass_k", -1)
    ctx.set_option("seq_event_stride", 0)
    ctx.set_option("pass2_tables", 1)
    ctx.set_option("pass2_tables_irregular_every", 0)
    ctx.set_option("fold_antithetic", 1)


def _run(n_paths, n_steps, n, **kw):
    from options_model_amd import _ffi
    return [_ffi.make_params(semantics="two_pass", n_paths=n_paths, n_steps=n_steps, seed=11, stream=i,
                             is_put=(i % 2 == 0), **kw) for i in range(n)]


@pytest.mark.parametrize("M,N,n", [
    (65_536, 9, 5),         # the smallest folded pricing; one time chunk
    (200_000, 50, 7),       # ragged tiles; 7 = 3 + 3 + 1, 2 + 2 + 2 + 1
    (1_000_000, 252, 6),    # the headline geometry; 6 = 4 + 2 at a width of 4
])
def test_every_member_of_a_group_returns_its_own_bits(gctx, M, N, n):
    ps = _run(M, N, n)
    singles = [gctx.price_american(p) for p in ps]
    assert all(s["folded"] == 1 for s in singles)
    widths = {}
    for k in (1, 2, 3, -1, 32):
        gctx.set_option("seq_two_pass_k", k)
        widths[k] = gctx.seq_group_width(ps)
        outs = gctx.price_american_seq(ps)   # n is not a multiple of K: a shorter last group or a single pricing left over
        for o, s in zip(outs, singles):
            _same(o, s)
    assert widths[1] == 1 and widths[2] == 2 and widths[3] == 3 and widths[32] == n
    assert 2 <= widths[-1] <= n              # all three sizes are grouped by default
    assert len({s["price"] for s in singles}) == n


def test_a_full_argument_block_and_a_pricing_left_over(gctx):
    """32 members fill the by-value argument block of the shared launches to its last slot (the other tests stop at 7,
    and never read the tail of the block); the 33rd pricing is left over and priced alone."""
    ps = _run(65_536, 9, 33)
    gctx.set_option("seq_two_pass_k", 32)
    assert gctx.seq_group_width(ps) == 32
    outs = gctx.price_american_seq(ps)
    assert len(outs) == 33
    for p, o in zip(ps, outs):
        _same(o, gctx.price_american(p))
    assert len({o["price"] for o in outs}) == 33


def test_mixed_sequence_groups_its_runs_and_leaves_the_rest_alone(gctx):
    from options_model_amd import _ffi
    run_a = _run(131_072, 30, 3)
    other_strike = _ffi.make_params(semantics="two_pass", n_paths=131_072, n_steps=30, seed=11, stream=40, K=95.0)
    unfolded = _ffi.make_params(semantics="two_pass", n_paths=4_000, n_steps=30, seed=11, stream=41)
    heston = _ffi.make_params(model="heston", is_put=False, semantics="two_pass", n_paths=131_072, n_steps=30, seed=11,
                              stream=42, heston_scheme="full_truncation")
    reference = _ffi.make_params(semantics="reference", n_paths=131_072, n_steps=30, seed=11, stream=43)
    run_b = [_ffi.make_params(semantics="two_pass", n_paths=131_072, n_steps=30, seed=12, stream=50 + i, is_put=(i != 1))
             for i in range(4)]
    ps = run_a + [other_strike, unfolded, heston, reference] + run_b
    gctx.set_option("seq_two_pass_k", -1)
    assert gctx.seq_group_width(ps) == 3                      # the run that starts the sequence ends at the other strike
    assert gctx.seq_group_width(ps[3:]) == 1 and gctx.seq_group_width(ps[7:]) == 4
    outs = gctx.price_american_seq(ps)
    for p, o in zip(ps, outs):
        _same(o, gctx.price_american(p))
    assert [o["folded"] for o in outs] == [1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1]


def test_sequences_that_do_not_qualify_are_not_grouped(gctx):
    import torch

    from options_model_amd import _ffi
    from options_model_amd.dist import _DevPtr
    ps = _run(100_000, 20, 4)
    base = [gctx.price_american(p) for p in ps]
    assert gctx.seq_group_width(ps) == 4
    for key, off in (("pass2_tables", 0), ("fold_antithetic", 0)):
        gctx.set_option(key, off)
        assert gctx.seq_group_width(ps) == 1
        outs = gctx.price_american_seq(ps)
        singles = [gctx.price_american(p) for p in ps]
        gctx.set_option(key, 1)
        for o, s, b in zip(outs, singles, base):
            _same(o, s)
            if key == "pass2_tables":      # the same decisions either way (test_gpu_pass2_tables.py)
                _same(o, b)
    # an all-reduce hook (one rank's identity): the moment table of every pricing goes through it between pass 1 and
    # the fits, so nothing is grouped
    stream = torch.cuda.Stream()
    c = _ffi.Context(0, stream=stream.cuda_stream)
    try:
        calls = []

        def ident(dptr, count):
            calls.append(count)
            torch.as_tensor(_DevPtr(dptr, count), device="cuda").add_(0.0)

        c.set_allreduce_hook(ident)
        assert c.seq_group_width(ps) == 1
        with torch.cuda.stream(stream):
            outs = c.price_american_seq(ps)
        c.set_allreduce_hook(None)
        assert calls.count(8 * 21) == len(ps)      # one moment table per pricing
        for o, b in zip(outs, base):
            _same(o, b)
    finally:
        c.close()


@pytest.mark.parametrize("M", [100_002, 200_000], ids=["vec1", "vec2"])
def test_irregular_steps_inside_a_shared_table_launch(gctx, M):
    ps = _run(M, 50, 5, sigma=0.4)
    gctx.set_option("pass2_tables_irregular_every", 5)
    gctx.set_option("seq_two_pass_k", 4)
    assert gctx.seq_group_width(ps) == 4
    outs = gctx.price_american_seq(ps)
    singles = [gctx.price_american(p) for p in ps]
    gctx.set_option("pass2_tables_irregular_every", 0)
    plain = [gctx.price_american(p) for p in ps]
    for o, s, q in zip(outs, singles, plain):
        _same(o, s)
        _same(o, q)    # the float64 fallback inside the table sweep takes the tables' decisions


def test_timed_members_keep_their_own_events(gctx):
    ps = _run(262_144, 100, 8)
    gctx.set_option("seq_two_pass_k", 8)
    gctx.set_option("seq_event_stride", 2)
    assert gctx.seq_group_width(ps) == 8
    outs = gctx.price_american_seq(ps)
    assert [o["timed"] for o in outs] == [1, 0, 1, 0, 1, 0, 1, 0]
    n = len(ps)
    for o in outs:
        if o["timed"]:
            assert o["ms_paths"] > 0 and o["ms_pass1"] > 0 and o["ms_pass2"] > 0
            assert o["ms_paths"] + o["ms_pass1"] + o["ms_pass2"] <= o["ms_total"] * n
        assert o["ms_lsm"] == pytest.approx(o["ms_total"] - o["ms_paths"], abs=1e-9)
    for p, o in zip(ps, outs):
        _same(o, gctx.price_american(p))


def test_no_room_for_the_group_halves_it_instead_of_failing():
    """Option "alloc_limit" stands in for a card without room: the group's matrices are ONE buffer, so a limit of three
    matrices refuses a group of 4 (the library falls back to groups of 2), one of 1.5 matrices refuses every group (one
    pricing at a time).  A fresh context and the tighter limit first: a buffer once allocated is large enough later."""
    from options_model_amd import _ffi
    M, N = 131_072, 30
    ps = _run(M, N, 5)
    matrix = 4 * (M // 2) * (N + 1)
    c = _ffi.Context(0)
    try:
        singles = [c.price_american(p) for p in ps]
        c.set_option("seq_two_pass_k", 4)
        for limit in (3 * matrix // 2, 3 * matrix):
            c.set_option("alloc_limit", limit)
            outs = c.price_american_seq(ps)
            for o, s in zip(outs, singles):
                _same(o, s)
        c.set_option("alloc_limit", 0)
        for o, s in zip(c.price_american_seq(ps), singles):   # and with room: groups of 4 + one left over
            _same(o, s)
    finally:
        c.set_option("alloc_limit", 0)
        c.close()


def test_a_larger_run_later_in_the_sequence_grows_the_group_buffers():
    """Two runs in one sequence, the second with larger matrices: the group buffers are released and allocated anew
    while the first run's groups may still be running in them."""
    from options_model_amd import _ffi
    ps = _run(65_536, 20, 3) + _run(262_144, 20, 4) + _run(65_536, 20, 2)
    c = _ffi.Context(0)
    try:
        assert c.seq_group_width(ps) == 3 and c.seq_group_width(ps[3:]) == 4
        outs = c.price_american_seq(ps)
        for p, o in zip(ps, outs):
            _same(o, c.price_american(p))
    finally:
        c.close()
