"""The device Philox4x32-10 forms each round's `hi ^ c ^ k` with one three-input XOR (omc_device.h: xor3, v_bitop3_b32
with truth table 0x96).  XOR is associative, so every output word must stay what the CPU oracle computes: bit-exact.

The rows put every operand position of the fused XOR through its corners: the product's high word (first operand), the
counter word carried over from the round before (second) and the round key (third).
"""
import numpy as np
import pytest

from oracle import cpu as orc

pytestmark = pytest.mark.gpu

W0, W1 = 0x9E3779B9, 0xBB67AE85  # the key schedule's increments (Weyl constants)
M32 = 0xFFFFFFFF
N_ROWS = 4096


def _rows():
    rng = np.random.default_rng(20240607)
    rows = []
    # 1. every word all-zero or all-ones, all 64 combinations of the six words
    for m in range(64):
        rows.append([M32 if (m >> b) & 1 else 0 for b in range(6)])
    # 2. one bit set alone, and one bit clear alone, at each of the 192 input bits
    for bit in range(192):
        r = [0] * 6
        r[bit // 32] = 1 << (bit % 32)
        rows.append(r)
        rows.append([w ^ M32 for w in r])
    # 3. keys whose schedule passes through 0xFFFFFFFF, 0 and 1 (the wrap of k0 += W0 / k1 += W1) at each of the
    #    rounds 1..9, both keys at once and each alone; counters random
    for rnd in range(1, 10):
        for d in (-1, 0, 1):
            k0 = (-rnd * W0 + d) & M32
            k1 = (-rnd * W1 + d) & M32
            for key in ((k0, k1), (k0, int(rng.integers(0, 2**32))), (int(rng.integers(0, 2**32)), k1)):
                for _ in range(4):
                    rows.append([int(x) for x in rng.integers(0, 2**32, size=4)] + list(key))
    # 4. the generators' counters (pair_lo, pair_hi, block, stream): 64 neighbouring pairs -- one wave -- straddling
    #    2^32 pairs, so pair_hi differs between neighbouring rows; seed-derived keys shared by the wave
    for block in (0, 1, 62, 251, M32):
        for stream in (0, 7, M32):
            k0, k1 = int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32))
            for lane in range(64):
                pair = (1 << 32) - 32 + lane
                rows.append([pair & M32, pair >> 32, block, stream, k0, k1])
    # 5. block and stream at 0xFFFFFFFF, each alone and both, under pair_hi on either side of a wrap of its own
    for pair_hi in (0, 1, M32):
        for block, stream in ((M32, 0), (0, M32), (M32, M32)):
            for _ in range(8):
                rows.append([int(rng.integers(0, 2**32)), pair_hi, block, stream,
                             int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32))])
    assert len(rows) <= N_ROWS
    a = np.array(rows, np.uint64).astype(np.uint32)
    # 6. random rows up to the full count (64 workgroups of the tap kernel)
    fill = rng.integers(0, 2**32, size=(N_ROWS - len(rows), 6), dtype=np.uint64).astype(np.uint32)
    return np.concatenate([a, fill])


@pytest.fixture(scope="module")
def rows_and_ref():
    inp = _rows()
    ref = np.stack([orc.philox4x32_10(row[:4], row[4:]) for row in inp])
    inp.setflags(write=False)
    ref.setflags(write=False)
    return inp, ref


def test_philox_xor3_rows_match_oracle(ctx, rows_and_ref):
    inp, ref = rows_and_ref
    assert inp.shape == (N_ROWS, 6)
    out = ctx.philox4x32_10(inp)
    bad = np.flatnonzero((out != ref).any(axis=1))
    assert bad.size == 0, (bad[:8], inp[bad[:8]], out[bad[:8]], ref[bad[:8]])


def test_philox_xor3_partial_workgroup(ctx, rows_and_ref):
    # a count that is no multiple of the launch's 64 threads: the same rows, the same words
    inp, ref = rows_and_ref
    n = 64 * 3 + 37
    assert np.array_equal(ctx.philox4x32_10(inp[:n]), ref[:n])
