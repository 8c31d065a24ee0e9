"""The cases of tests/test_gpu_heston_qe_consumers.py: the laws, shapes, coordinates, barrier levels, dividend schedules and jump
laws at which every kernel that takes heston_pair_step<3> (the QE scheme) is run with work to do.
TEST INFRASTRUCTURE ONLY.

tests/test_heston_qe_consumers_cpu.py restates every case in float64 (heston_qe_ref.paths on the C oracle's normals, which are
the device's) and asserts what the GPU tests rely on, so that none of them can pass empty: a barrier that some paths meet and
some do not, payoffs on both sides of the strike, exponential and quadratic lanes in one wave (set B), jump cells and cells
without, dividends that leave every path above 0 (and one that does not, on purpose).

Barrier levels.  A GPU test compares with the encoder on the device's OWN matrix, so it needs no margin; the CPU test, which
sees the float64 restatement only, does: `tail` levels have NO restated spot within relative MARGIN of them (the margin of
test_barrier_no_path_hits), so the device's float32 spots (5e-5 from the restatement) hit exactly where the restatement does.
With 10^5 spots in a matrix such a level exists in the tails only, where a handful of paths hit; `BULK` (the levels of
tests/test_gpu_barrier.py) is run besides wherever n_paths >= 1000: there the CPU test counts the paths that pass the level by
more than the margin and those that stay more than the margin away, and asks for at least 1 % of each.
"""
import functools

import numpy as np

from helpers import heston_qe_ref as qe

S0, R, T = qe.MARKET["S0"], qe.MARKET["r"], qe.MARKET["T"]
K = 100.0
QE = 3
LAWS = dict(qe.SETS)
MARGIN = 1e-3
BULK = (90.0, 112.0)          # (down, up) of tests/test_gpu_barrier.py
WAVE = 64


def law_args(law):
    return [LAWS[law][k] for k in ("v0", "kappa", "theta", "xi", "rho")]


# ---------------------------------------------------------------------------------------------- the restatement of a case
@functools.lru_cache(maxsize=4)
def restated(law, M, N, seed, stream, off=0, rate=R, t=T):
    """heston_qe_ref.paths on the oracle's normals at the case's coordinates -> dict S, V [N+1][M], expo [N][M] (float64)"""
    from oracle import cpu as orc
    z1, z2 = qe.pair_view(orc.gbm_normals(M // 2, 2 * N, seed, stream, off))
    h = LAWS[law]
    return qe.paths(z1, z2, S0, h["v0"], rate, t, h["kappa"], h["theta"], h["xi"], h["rho"])


def store_vec(M):
    """pairs per thread of the full-storage generators at the default width hint and ld = n_paths (store_vec_width)"""
    P = M // 2
    return 4 if P % 4 == 0 else 2 if P % 2 == 0 else 1


def wave_any(cells, M, vec=1):
    """cells bool [rows][M] (antithetic layout) -> [rows][waves]: does any lane of the wave (64 threads x vec pairs, both
    partners of a pair in one lane) hold a True"""
    P = M // 2
    pair = cells[:, :P] | cells[:, P:]
    per = WAVE * vec
    n = -(-P // per)
    pad = np.zeros((pair.shape[0], n * per - P), bool)
    return np.concatenate([pair, pad], axis=1).reshape(pair.shape[0], n, per).any(axis=2)


def mixed_waves(expo, M, vec=1):
    """the (step, wave) cells in which one lane is exponential and another quadratic (a partly filled wave counts its
    lanes only)"""
    return wave_any(expo, M, vec) & wave_any(~expo, M, vec)


def expects_mixed(M, N):
    """At step 1 every lane holds v0, hence one psi = s2 / m^2 and one branch (set B: exponential down to about 8 steps a
    year, psi = 6.1 at dt = 1 and 3.4 at dt = 0.2; quadratic at 50): a wave can mix from step 2 on only, once the lanes'
    variances have parted.  A case is expected to show a mixed wave when it has a second step and at least one full wave
    of pairs."""
    return N >= 2 and M // 2 >= WAVE


# ---------------------------------------------------------------------------------------------- barrier
# name -> law, M, N, seed, stream, pair_offset, tail = (down, up).  The levels were searched on the restatement (the highest
# down level / lowest up level with the margin free of spots, among the gaps between the sorted per-path extremes).
def _b(law, M, N, seed, stream, off, down, up):
    return dict(law=law, M=M, N=N, seed=seed, stream=stream, off=off, tail=(down, up))


EURO_SEED, EURO_OFFSET = 20240611, 321   # the coordinates of tests/test_gpu_european_sums.py
BARRIER_ENCODE = {
    "enc-B-50": _b("B", 4096, 50, 42, 3, 0, 32.733, 161.49),          # 31 / 3 of 4,096 paths hit
    "enc-B-51": _b("B", 4096, 51, 42, 3, 0, 39.93, 166.69),           # 56 / 2
    "enc-C-50": _b("C", 4096, 50, 42, 3, 0, 51.324, 152.32),          # 11 / 6
    "enc-C-51": _b("C", 4096, 51, 42, 3, 0, 51.891, 155.03),          # 11 / 4
}
BARRIER_EURO = {
    # (the one-pair and four-pair shapes: stream 15 where stream 13 sends no single partner through a level on its side of S0)
    "euro-B-2x5": _b("B", 2, 5, EURO_SEED, 15, EURO_OFFSET, 83.668, 107.97),           # 1 / 1
    "euro-B-8x5": _b("B", 8, 5, EURO_SEED, 13, EURO_OFFSET, 97.807, 109.52),           # 1 / 6
    "euro-B-1026x5": _b("B", 1026, 5, EURO_SEED, 13, EURO_OFFSET, 68.512, 132.63),     # 63 / 27
    "euro-B-2048x5": _b("B", 2048, 5, EURO_SEED, 13, EURO_OFFSET, 66.788, 139.56),     # 124 / 30
    "euro-B-2056x5": _b("B", 2056, 5, EURO_SEED, 13, EURO_OFFSET, 66.788, 139.56),     # 125 / 30
    "euro-B-2x9": _b("B", 2, 9, EURO_SEED, 15, EURO_OFFSET, 79.407, 109.65),           # 1 / 1
    "euro-B-8x9": _b("B", 8, 9, EURO_SEED, 13, EURO_OFFSET, 96.512, 107.24),           # 3 / 6
    "euro-B-1026x9": _b("B", 1026, 9, EURO_SEED, 13, EURO_OFFSET, 67.091, 134.03),     # 63 / 18
    "euro-B-2048x9": _b("B", 2048, 9, EURO_SEED, 13, EURO_OFFSET, 59.611, 134.03),     # 97 / 42
    "euro-B-2056x9": _b("B", 2056, 9, EURO_SEED, 13, EURO_OFFSET, 59.611, 134.03),     # 97 / 42
    "euro-B-131074x5": _b("B", 131074, 5, EURO_SEED, 13, EURO_OFFSET, 22.306, 184.33),  # 276 / 25 of 131,074
    "euro-C-2x5": _b("C", 2, 5, EURO_SEED, 15, EURO_OFFSET, 91.123, 112.33),           # 1 / 1
    "euro-C-8x5": _b("C", 8, 5, EURO_SEED, 13, EURO_OFFSET, 96.869, 108.48),           # 1 / 4
    "euro-C-1026x5": _b("C", 1026, 5, EURO_SEED, 13, EURO_OFFSET, 80.896, 125.96),     # 47 / 26
    "euro-C-2048x5": _b("C", 2048, 5, EURO_SEED, 13, EURO_OFFSET, 80.969, 128.28),     # 106 / 48
    "euro-C-2056x5": _b("C", 2056, 5, EURO_SEED, 13, EURO_OFFSET, 80.969, 128.28),     # 106 / 48
    "euro-C-2x9": _b("C", 2, 9, EURO_SEED, 15, EURO_OFFSET, 89.092, 109.5),            # 1 / 1
    "euro-C-8x9": _b("C", 8, 9, EURO_SEED, 13, EURO_OFFSET, 95.433, 106.49),           # 1 / 5
    "euro-C-1026x9": _b("C", 1026, 9, EURO_SEED, 13, EURO_OFFSET, 79.657, 130.66),     # 46 / 17
    "euro-C-2048x9": _b("C", 2048, 9, EURO_SEED, 13, EURO_OFFSET, 70.402, 135.31),     # 43 / 15
    "euro-C-2056x9": _b("C", 2056, 9, EURO_SEED, 13, EURO_OFFSET, 70.402, 135.31),     # 43 / 15
    "euro-C-131074x5": _b("C", 131074, 5, EURO_SEED, 13, EURO_OFFSET, 45.401, 175.11),  # 163 / 14
}
BARRIER_AMERICAN = {
    "amer-B": _b("B", 16384, 40, 42, 20, 0, 22.635, 166.01),          # 46 / 11 of 16,384 (stream 12: one path above)
    "amer-C": _b("C", 16384, 40, 42, 12, 0, 42.215, 159.45),          # 15 / 16
}
BARRIER_SHARD = {
    "shard-B": _b("B", 4096, 33, 42, 61, 0, 35.894, 162.98),          # 33 / 7
    "shard-C": _b("C", 4096, 33, 42, 61, 0, 51.375, 143.94),          # 12 / 17
}


def barrier_cases():
    out = {}
    for group in (BARRIER_ENCODE, BARRIER_EURO, BARRIER_AMERICAN, BARRIER_SHARD):
        out.update(group)
    return out


def level_sets(case):
    """the (down, up) pairs a GPU test runs the case at"""
    return [case["tail"]] + ([BULK] if case["M"] >= 1000 else [])


def hit_steps(S, direction, H):
    """first step 1..N with S <= H (down) / >= H (up) per column of a float64 matrix; N + 1: never"""
    hit = S[1:] <= H if direction == "down" else S[1:] >= H
    return np.where(hit.any(axis=0), hit.argmax(axis=0) + 1, S.shape[0])


def nearest_spot(S, H):
    """the smallest relative distance of a spot of rows 1..N from H"""
    return float(np.abs(S[1:] / H - 1.0).min())


# ---------------------------------------------------------------------------------------------- European sums
EURO_STREAM = 3
EURO_BATCH = [(514, 5), (4098, 9), (254, 4), (2, 1)]   # the antithetic shapes of the batch test, streams 4 + i


def euro_cases():
    """(law, M, N, stream) of omc_price_european and its batch, on (EURO_SEED, stream, EURO_OFFSET)"""
    import test_gpu_european_sums as es
    out = []
    for law in LAWS:
        out += [(law, M, N, EURO_STREAM) for N in es.EURO_N for M in es.EURO_M] + [(law,) + es.EURO_BIG + (EURO_STREAM,)]
        out += [(law, M, N, 4 + i) for i, (M, N) in enumerate(EURO_BATCH)]
    return out


STRIKE_STREAM = 23
SURFACE = dict(N=7, expiries=[0.25, 0.5, 1.0], streams=[31, 32, 33])


# ---------------------------------------------------------------------------------------------- dividends
DIV_SEED, DIV_STREAM = 77, 2
DIV_LAWS = ("B", "C")


def div_yield(law):
    return 0.025 if law == "B" else -0.01   # a yield of either sign


# a cash dividend at mid-life that takes a share of the paths to 0: (law, cash amount); 40,000 x 20 on (31, 4), yield 0.03
DIV_ZERO = dict(M=40_000, N=20, seed=31, stream=4, q=0.03, cash={"B": 0.9 * S0, "C": 1.0 * S0})


def mixed_schedule(N):
    """test_gpu_dividends.mixed_schedule(p, "heston") without a params struct: -> (dividends, ex steps)"""
    dt = T / N
    steps = sorted({k for k in (1, 2, 3, N) if 1 <= k <= N})
    amounts = [(0.9, "cash"), (0.015, "proportional"), (1.3, "cash"), (0.02, "proportional")][:len(steps)]
    divs = [((k - 0.5) * dt,) + a for k, a in zip(steps, amounts)]
    divs.append((divs[-1][0], 0.4, "cash"))
    return divs[::-1], steps


# ---------------------------------------------------------------------------------------------- jumps
JUMP_LAWS = ("B", "C")
JUMP_COORDS = ((True, 2, 0), (False, 3, 777))   # (is_put, stream, pair_offset) of tests/test_gpu_jumps.py, seed 77
JUMP_SEED = 77
BALLOT_SHAPE = (1_026, 7)   # 513 pairs, one per thread: eight full waves and a ninth of one lane


def jump_table(N, lam, mu, sj, q):
    from helpers import jump_ref as jr
    thr, kappa, rate, _ = jr.table(lam, mu, sj, R, q, T, N)
    return thr, kappa, rate


@functools.lru_cache(maxsize=None)
def jump_counts(M, N, stream, off, thr):
    """the jump counts [N+1][P] of a case from the oracle's Philox (the sizes are not needed here)"""
    from helpers import jump_ref as jr
    from oracle import cpu as orc
    P, ncb = M // 2, (N + 3) // 4
    key = (JUMP_SEED & 0xFFFFFFFF, (JUMP_SEED >> 32) & 0xFFFFFFFF)
    words = np.zeros((P, 4 * ncb + 1), np.int64)
    for p in range(P):
        pair = off + p
        for cb in range(ncb):
            words[p, 4 * cb + 1:4 * cb + 5] = orc.philox4x32_10((pair & 0xFFFFFFFF, pair >> 32, jr.COUNT_TAG | cb, stream), key)
    n = jr.count(words.T[:N + 1] >> 8, np.array(thr, np.uint32))
    n[0] = 0
    return n


# ---------------------------------------------------------------------------------------------- American pricing paths
BATCH_SHAPES = [(514, 5), (4096, 9), (254, 4)]
CHAIN = dict(M=16_384, N=12, strikes=(95.0, 100.0, 105.0), puts=(True, False, True))
SEQ = dict(M=16_384, N=9, n=3)
GREEKS = dict(M=20_004, N=37, seed=42, stream=0)
FUZZ_M = [2, 66, 1026, 4098, 8190, 12_290]   # at most 12,290 paths
FUZZ_N_MAX = 40


def fuzz_laws(n, seed):
    """n laws of heston_qe_ref.fuzz_cases (every third violates Feller) with a shape of their own: at most 12,290 paths
    and 40 steps"""
    rng = np.random.default_rng(seed + 1)
    out = []
    for c in qe.fuzz_cases(n, seed):
        c = dict(c, M=int(rng.choice(FUZZ_M)), N=min(c["N"], FUZZ_N_MAX), is_put=bool(rng.integers(0, 2)),
                 nk=int(rng.integers(1, 25)), n_exp=int(rng.integers(1, 5)), bump=float(rng.choice([0.001, 0.01, 0.1])),
                 K=float(rng.choice([0.9, 1.0, 1.1])) * c["S0"], M_greeks=int(rng.choice([254, 1026, 4098, 12_290])))
        out.append(c)
    return out


# ---------------------------------------------------------------------------------------------- every case, for the branch checks
AMERICAN_SEED = qe.SEED   # batch, chain and sequence: (qe.SEED, stream 4 + i / 6 / i)


def jump_rate(N):
    import test_gpu_jumps as gj
    return jump_table(N, gj.lam_of(N), gj.MU, gj.SJ, gj.Q)[2]


def set_cases():
    """Every (label, law, M, N, seed, stream, pair_offset, drift rate, T) a GPU test generates QE paths at, one entry per
    matrix: what the branch conditions of the three sets are asserted on."""
    import test_gpu_dividends as gd
    import test_gpu_european_sums as es
    out = [("barrier " + name, c["law"], c["M"], c["N"], c["seed"], c["stream"], c["off"], R, T) for name, c in barrier_cases().items()]
    out += [("european", law, M, N, EURO_SEED, stream, EURO_OFFSET, R, T) for law, M, N, stream in euro_cases()]
    for law in LAWS:
        out += [("strikes", law, M, N, EURO_SEED, STRIKE_STREAM, 0, R, T) for N in es.STRIKE_N for M in es.STRIKE_M]
        out += [("surface", law, es.SURFACE_M, SURFACE["N"], EURO_SEED, s, 0, R, t) for t, s in zip(SURFACE["expiries"], SURFACE["streams"])]
    for law in DIV_LAWS:
        out += [("dividends", law, M, N, DIV_SEED, DIV_STREAM, 0, R - div_yield(law), T) for M, N in gd.SHAPES]
        z = DIV_ZERO
        out.append(("dividends to zero", law, z["M"], z["N"], z["seed"], z["stream"], 0, R - z["q"], T))
    for law in JUMP_LAWS:
        out += [("jumps", law, M, N, JUMP_SEED, stream, off, jump_rate(N), T) for M, N in gd.SHAPES[:4] for _, stream, off in JUMP_COORDS]
    for law in ("B", "C"):
        out += [("batch", law, M, N, AMERICAN_SEED, 4 + i, 0, R, T) for i, (M, N) in enumerate(BATCH_SHAPES)]
        out.append(("chain", law, CHAIN["M"], CHAIN["N"], AMERICAN_SEED, 6, 0, R, T))
        out += [("sequence", law, SEQ["M"], SEQ["N"], AMERICAN_SEED, i, 0, R, T) for i in range(SEQ["n"])]
    out.append(("greeks", "C", GREEKS["M"], GREEKS["N"], GREEKS["seed"], GREEKS["stream"], 0, R, T))
    return out
