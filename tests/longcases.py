"""The named blocks of the long periods' GPU tests (tests/test_gpu_long_period_*.py), built here so that
tests/test_longperiodmodel.py can prove, without a GPU, that every one has the edge it is named for."""
import functools

import numpy as np

import periodcases as pc

TILE = 16384
LENGTH_PERIODS = (4097, 16383, 16384, 16385, 65539, (1 << 20) + 1)
LENGTHS_N = (1 << 21) + 4096
# name -> position: a 16-byte load's, a thread's 64 positions', a wave's 4096, a tile's (twice), the last position
ONE_STRETCH = [(4097, "random"), (8192, "random"), (65537, "random"), (8192, "text")]
SEAMS_AT ={"load": 16, "thread": 192, "wave": 4096, "tile": TILE, "far tile": 13 * TILE}


def seams(p, n=LENGTHS_N):
    """The seams of tests/periodcases.py SEAMS, moved behind p (breaks lie at q >= p): positions that are a load's, a
    thread's, a wave's and a tile's first, and the block's last."""
    first = (p // TILE + 1) * TILE
    out = {name: first + at for name, at in SEAMS_AT.items() if first + at < n - 1}
    out["last"] = n - 1
    return out


def seam_block(p, delta, n=LENGTHS_N):
    """A stretch of period p over n bytes with a break at seam + delta for every seam."""
    T = pc.stretch(p, n)
    at = sorted({q + delta for q in seams(p, n).values() if p <= q + delta < n})
    return pc.with_breaks(T, p, at), at


def noise(n, seed):
    """Random bytes 0 ... 255."""
    return np.random.default_rng([29, n, seed]).integers(0, 256, n).astype(np.uint8)


def text(n, seed):
    from bwtc_amd import synth
    return synth.gen_text(n, seed)


@functools.lru_cache(maxsize=None)
def one_stretch(p, inside="random"):
    """One stretch of 16 periods of a primitive unit in the middle of random bytes or of the generator's text: at least
    1 MiB in all."""
    L = 16 * p
    side = max((1 << 20) - L, 8 * p) // 2
    make = noise if inside == "random" else text
    d = pc.cat(make(side, 1), pc.stretch(p, L), [0], make(side, 2))
    d.setflags(write=False)
    return d


def tie_blocks(p):
    """tests/periodcases.py tie_blocks() with stretches of 9 p + 5 bytes (the case of 64 short stretches left out: 400
    bytes hold no long period): rising and falling types, the block's end, equal (type, k) from 2 and 3 stretches."""
    return [(what, d) for what, d in pc.tie_blocks(p, 9 * p + 5) if "64" not in what]


def worth_block(p, delta):
    """Noise with one planted stretch of exactly 8 p + delta periodic characters: the worth threshold."""
    return pc.gate_block(p, 8 * p + delta, n=8 * p + 120000)


def forced_block(p):
    """A stretch of 3 p bytes in noise: too short for the votes' worth, long enough for a named period's gate."""
    return pc.cat(noise(70000, 3), pc.stretch(p, 3 * p), [0], noise(70000, 4))


def division_block(p):
    """A stretch of 12 periods of p = 2^2 5^2 41 or 2^13 in noise: the winner is the true period, and the division tries
    every prime factor in vain."""
    return pc.cat(noise(50000, 5), pc.stretch(p, 12 * p), [0], noise(50000, 6))


@functools.lru_cache(maxsize=None)
def multiple_block(q):
    """4 MiB of random bytes with a 3 MiB stretch of period q: a list of more than 2^21 entries (the sorter's dense route).
    With its groups' members by the suffix number's low 8 bits (longperiodmodel.window_order_list) the votes name
    lcm(q, 256) and the division finds q; the sorter's own list of this block is in position order and votes for q."""
    d = np.random.default_rng(11).integers(0, 256, 4 << 20).astype(np.uint8)
    d[1 << 19:(1 << 19) + (3 << 20)] = pc.stretch(q, 3 << 20)
    d.setflags(write=False)
    return d


MULTIPLE_OF = {4100: 64 * 4100, 1025: 256 * 1025}          # the winner over window_order_list(multiple_block(q)): lcm(q, 256) = 262 400 for both


@functools.lru_cache(maxsize=None)
def back_to_back():
    """64 KiB of text 32 times: 2 MiB of period 65 536."""
    d = np.tile(text(1 << 16, 5), 32)
    d.setflags(write=False)
    return d


def long_and_short():
    """A stretch of period 9 and one of period 5000 in noise (BWTC_HIP_MULTI: two period steps)."""
    return pc.cat(noise(40000, 7), pc.stretch(9, 60000), [0], noise(40000, 8), pc.stretch(5000, 60000), [1], noise(40000, 9))


def random_block(it):
    """Block `it` of the 40: noise with one stretch of 9 ... 12 periods of p, 4097 <= p <= 40 000 -> (block, p, the
    stretch's length)."""
    rng = np.random.default_rng([20260101, it])
    p = int(rng.integers(4097, 40001))
    L = int(rng.integers(9 * p, 12 * p + 1))
    before, behind = int(rng.integers(100, 60000)), int(rng.integers(100, 60000))
    d = pc.cat(noise(before, 2 * it), pc.stretch(p, L, it % 3, int(rng.integers(0, p))), [int(rng.integers(0, 2)) * 255], noise(behind, 2 * it + 1))
    return d, p, L


def controls():
    """(name, block): blocks that hold no long period -- the switch changes nothing."""
    return [("period 9", pc.stretch(9, 300000)), ("period 4096", pc.stretch(4096, 1 << 19)), ("text", text(1 << 19, 3))]
