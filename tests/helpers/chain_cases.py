"""Seeded random option chains for tests/test_gpu_chain_fuzz.py: one expiry, 1 .. 12 quotes, against their single calls.

Whatever the seed, the first cases deal what the sweep is there for: folded and full storage (the storage rule switches at
65,536 paths), both vector widths of the folded sweeps (stored columns a multiple of four or not), chains of one side, of
both sides, with a duplicated quote, of one entry and of twelve."""
import numpy as np

FOLD_MIN_PATHS = 65_536  # options_model_amd: folded storage from here on (GBM, option "fold_antithetic" = 1)


def chain_cases(n, seed):
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        # sizes: [2, 300k] even; the first eight alternate storage and alignment
        if i % 8 == 0:
            M = int(rng.integers(FOLD_MIN_PATHS // 8, 300_000 // 8 + 1)) * 8          # folded, 16-byte loads
        elif i % 8 in (1, 5):
            M = int(rng.integers(1, FOLD_MIN_PATHS // 2)) * 2                          # full storage
        elif i % 8 == 2:
            M = int(rng.integers(FOLD_MIN_PATHS // 8, 300_000 // 8)) * 8 + 2           # folded, scalar loads
        elif i % 8 == 3:
            M = FOLD_MIN_PATHS if i == 3 else FOLD_MIN_PATHS - 2                       # either side of the rule
        else:
            M = int(rng.integers(1, 150_001)) * 2
        N = int(rng.integers(2, 81))
        S0 = float(rng.uniform(20.0, 200.0))
        n_entries = (1, 12, 7, 5)[i] if i < 4 else int(rng.integers(1, 13))
        strikes = [float(S0 * rng.uniform(0.5, 1.6)) for _ in range(n_entries)]
        if i % 4 == 0:
            sides = [True] * n_entries
        elif i % 4 == 1:
            sides = [bool(j % 2) for j in range(n_entries)]
        else:
            sides = [bool(x) for x in rng.integers(0, 2, n_entries)]
        if n_entries >= 3 and i % 2 == 0:  # a duplicated quote, not next to its twin
            strikes[-1], sides[-1] = strikes[0], sides[0]
        cases.append(dict(M=M, N=N, S0=S0, r=float(rng.uniform(0.0, 0.1)), sigma=float(rng.uniform(0.1, 0.6)),
                          T=float(rng.uniform(0.1, 2.0)), strikes=strikes, sides=sides, seed=int(rng.integers(1, 2 ** 31)),
                          chain_k=(-1, 1, 2, 3, 16)[i % 5]))
    return cases


def is_folded(case):
    return case["M"] >= FOLD_MIN_PATHS


def has_duplicate(case):
    quotes = list(zip(case["strikes"], case["sides"]))
    return len(set(quotes)) < len(quotes)
