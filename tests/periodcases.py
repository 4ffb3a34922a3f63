"""The blocks of the period step's GPU tests (tests/test_gpu_period_lengths.py, tests/test_gpu_period_step.py), built
here so that tests/test_periodmodel.py can prove, without a GPU, that every named block has the edge it is named for."""
import numpy as np

TILE = 16384
PERIODS = (1, 2, 3, 7, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096)
SEAM_N = 17 * TILE + 3
# name -> position: a 16-byte load's, a thread's 64 positions', a wave's 4096, a tile's (twice), the last position
SEAMS = {"load": TILE + 4096 + 16, "thread": TILE + 4096 + 192, "wave": 2 * TILE + 4096, "tile": 3 * TILE, "far tile": 16 * TILE,
         "last": SEAM_N - 1}


def lengths_of(p):
    """The block lengths of the period-length pass's cases."""
    return sorted({1, p, p + 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1, SEAM_N, (1 << 20) + 3})


def unit(p, seed):
    """p bytes in 2 ... 250, the last one 251 and nowhere else: a primitive unit (no shorter period)."""
    u = np.random.default_rng([7, p, seed]).integers(2, 251, p).astype(np.uint8)
    u[-1] = 251
    return u


def stretch(p, n, seed=0, phase=0):
    """n bytes of period p."""
    u = np.roll(unit(p, seed), -phase)
    return np.tile(u, n // p + 1)[:n].copy()


def with_breaks(T, p, breaks):
    """T, a stretch of period p, with exactly the positions `breaks` (each >= p) made breaks: from q on the unit's byte
    at q mod p is another one."""
    T = T.copy()
    for q in sorted(set(breaks)):
        assert p <= q < T.size
        T[q::p] = (int(T[q]) + 1) % 256
    return T


def seam_breaks(p, delta):
    """Break positions at seam + delta for every seam (those that can be breaks: q >= p)."""
    return sorted({q + delta for q in SEAMS.values() if p <= q + delta < SEAM_N})


def before_seam_breaks(p):
    """Breaks exactly p before the seams: the first break at or behind s + p is looked for across the seam."""
    return sorted({q - p for q in SEAMS.values() if q - p >= p})


def spaced_breaks(p):
    """Breaks p - 1, p and p + 1 apart, from position 5 p + 11 on."""
    out, q = [], 5 * p + 11
    for gap in (p - 1, p, p + 1, p, p - 1, p + 1, p + 1):
        out.append(q)
        q += max(gap, 1)
    return out


def two_symbols(n, seed):
    return np.random.default_rng([11, n, seed]).integers(0, 2, n).astype(np.uint8) + 97


# ---- the step's blocks -------------------------------------------------------------------------

def filler(n, seed):
    """Noise over 252 ... 255 and 0 ... 1: symbols no unit holds, so no stretch goes on into it by chance."""
    return np.array([252, 253, 254, 255, 0, 1], np.uint8)[np.random.default_rng([13, n, seed]).integers(0, 6, n)]


def cat(*parts):
    return np.concatenate([np.asarray(q, np.uint8).ravel() for q in parts])


def tie_blocks(p, L):
    """(name, block): stretches of L bytes of one unit of period p that end in a smaller byte, a larger byte, the block's
    end and each other; equal (type, k) from 2, 3 and 64 stretches; units that are rotations of one another.
    (The sorter sees a block reversed or not; these are written as the sorter's T and the tests hold every block to the
    oracle, so a reversal changes which member is which, not what is covered: see the premises in test_periodmodel.)"""
    S = stretch(p, L)
    nxt = int(unit(p, 0)[L % p])                   # the byte the period asks for behind S
    low, high = nxt - 1, nxt + 1
    out = [("ends below, above and at the end", cat(filler(300, 1), S, [low], filler(300, 2), S, [high], filler(300, 3), S)),
           ("ends in each other", cat(S, stretch(p, L, 1), S, stretch(p, L, 2), [low], S))]
    for copies in (2, 3, 64):
        parts = []
        for i in range(copies):
            parts += [S[:min(L, 400)] if copies == 64 else S, [low if i % 2 else high], filler(40, 20 + i)]
        out.append(("equal (type, k) from %d stretches" % copies, cat(*parts)))
    out.append(("rotations of one unit", cat(S, [0], stretch(p, L, 0, 1), [255], stretch(p, L, 0, p // 2), [0], S)))
    return out


def nonprimitive_block(L):
    """abab...: period 2, sorted with p forced to 4."""
    return cat(filler(100, 5), np.tile(np.frombuffer(b"ab", np.uint8), L // 2), [1], filler(100, 6), np.tile(np.frombuffer(b"ab", np.uint8), L // 2))


def unit_of_five(p):
    """p >= 5 bytes over A, C, G, T with one Z at the end: five symbols whatever p is, so the depth at which the rounds
    begin does not depend on p."""
    u = np.array([65, 67, 71, 84], np.uint8)[np.random.default_rng([23, p]).integers(0, 4, p)]
    u[:4] = [65, 67, 71, 84]
    u[-1] = 90
    return u


def gate_block(p, periodic, n=200000, seed=3):
    """Noise over 1 ... 255 with one planted stretch of exactly `periodic` p-periodic characters (0: none planted): the
    bytes before and behind it are made to disagree with the period."""
    d = np.random.default_rng([17, seed]).integers(1, 256, n).astype(np.uint8)
    if periodic:
        u = np.random.default_rng([19, p]).integers(1, 256, p).astype(np.uint8)
        a, b = 50000, 50000 + periodic
        d[a:b] = np.tile(u, periodic // p + 1)[:periodic]
        if periodic > p:
            d[b] = d[b - p] % 255 + 1                    # (another byte of 1 ... 255)
            d[a - 1] = d[a - 1 + p] % 255 + 1
    return d


def gate_block_longest(p, periodic):
    """The longest p-periodic stretch of gate_block(p, periodic) that begins outside the planted one."""
    from periodmodel import period_lengths_np
    k = period_lengths_np(gate_block(p, periodic), p)[0].copy()
    k[50000:50000 + max(periodic, 1)] = 0
    return int(k.max())


def random_block(it):
    """Block `it` of the randomised case: stretches of mixed periods (1 included) and noise, 300 ... 300 000 bytes."""
    rng = np.random.default_rng([20250101, it])
    n = int(300 * 1000 ** rng.random())
    periods = [1, 2, 3, 5, 9, 16, 17, 64, 100, 257]
    parts, have = [], 0
    while have < n:
        kind = rng.random()
        if kind < 0.3:
            q = rng.integers(0, 256, int(rng.integers(1, 200))).astype(np.uint8)
        else:
            p = int(rng.choice(periods))
            L = int(rng.choice([p, 2 * p + 1, 70, 300, 5000, 70000]))
            q = stretch(p, L, int(rng.integers(0, 2)), int(rng.integers(0, p)))
        parts.append(q)
        have += q.size
    d = np.concatenate(parts)[:n]
    if it % 4 == 0:
        d = np.concatenate([d[:n // 2], d[:n // 2]])
    return d, (1, 2, 8, 256)[it % 4]
