"""The blocks of the mixed steps' tests (tests/test_gpu_period_proper.py, tests/test_gpu_mixed_steps.py), built here so
that tests/test_mixedmodel.py can prove, without a GPU, that every named block has the edge it is named for: the run
exceeds the depth, the proper stretch passes the gate, the votes reach max(256, n / 64) where the case is voted.

The sorter sees a block reversed or not.  A run reversed is the same run and a stretch reversed a stretch of the same
period and length, so the premises are proved for the block and for its reverse."""
import numpy as np

import mixedmodel
import periodcases as pc
from periodmodel import PERIOD_MAX, period_lengths_np

TILE = pc.TILE


# ---- the model's texts (tests/test_mixedmodel.py) -------------------------------------------

def model_text(seed, n=None):
    """(text, p): runs, stretches of one period p in 2 ... 20 (units a...ab included: an inner run below p), and noise, over
    2 ... 5 symbols, 40 ... 160 bytes."""
    rng = np.random.default_rng([31, seed])
    sigma = int(rng.integers(2, 6))
    p = int(rng.integers(2, 21))
    n = int(rng.integers(40, 161)) if n is None else n
    if rng.random() < 0.4:
        u = np.full(p, rng.integers(0, sigma), np.uint8)             # a...ab
        u[-1] = (u[0] + 1 + rng.integers(0, sigma - 1)) % sigma
    else:
        u = rng.integers(0, sigma, p).astype(np.uint8)
    parts, have = [], 0
    while have < n:
        kind = rng.random()
        if kind < 0.3:
            q = np.full(int(rng.integers(1, 40)), rng.integers(0, sigma), np.uint8)
        elif kind < 0.7:
            q = np.tile(np.roll(u, -int(rng.integers(0, p))), 8)[:int(rng.integers(p, 6 * p + 2))]
        else:
            q = rng.integers(0, sigma, int(rng.integers(1, 12))).astype(np.uint8)
        parts.append(q)
        have += q.size
    return bytes((np.concatenate(parts)[:n] + 97).astype(np.uint8)), p


def runs_only_text(seed):
    """Runs and noise over 2 ... 4 symbols: no stretch of a period 2 ... 20 is planted."""
    rng = np.random.default_rng([37, seed])
    sigma = int(rng.integers(2, 5))
    parts = []
    for _ in range(int(rng.integers(3, 9))):
        parts.append(np.full(int(rng.integers(1, 50)), rng.integers(0, sigma), np.uint8))
        parts.append(rng.integers(0, sigma, int(rng.integers(1, 8))).astype(np.uint8))
    return bytes((np.concatenate(parts) + 97).astype(np.uint8))


# ---- the pass's blocks (tests/test_gpu_period_proper.py) ----------------------------------------

def proper_blocks(p):
    """(name, T) for the stretch-length pass with its second maximum, period p >= 2."""
    S = pc.stretch(p, 3 * TILE + 1000)
    out = []
    T = S.copy(); T[2000:32000] = 7
    out.append(("the longest stretch is a run", T))
    for delta in (-1, 0, 1):
        T = pc.cat(pc.filler(500, delta + 5), np.full(max(p + delta, 1), 9, np.uint8), [200], pc.stretch(p, 5 * p + 300, 1), pc.filler(300, 9))
        out.append(("a run of p %+d bytes beside a stretch" % delta, T))
    # the one proper position of the block, s, on the last byte of a 64-byte chunk, of a wave's span, of a tile, and at
    # n - 2: equal bytes up to s, another byte from s + 1 on
    n = 3 * TILE + 1000
    for name, s in (("chunk", TILE + 4096 + 63), ("wave", TILE + 4095), ("tile", 2 * TILE - 1), ("n - 2", n - 2)):
        T = np.full(n, 5, np.uint8); T[s + 1:] = 6
        out.append(("the proper position on the last byte of a %s" % name, T))
        T = S.copy(); T[:s + 1] = 1                                     # ... and with a stretch behind it
        out.append(("the run's last byte on the last byte of a %s, a stretch behind" % name, T))
    out.append(("all equal", np.full(2 * TILE + 5, 3, np.uint8)))
    for n in sorted({1, 2, p - 1, p, p + 1} - {0}):
        out.append(("%d bytes of noise" % n, pc.two_symbols(n, p)))
        out.append(("%d equal bytes" % n, np.full(n, 8, np.uint8)))
    out.append(("noise over two symbols", pc.two_symbols(2 * TILE + 1, 3)))
    out.append(("a stretch with breaks at the seams", pc.with_breaks(pc.stretch(p, pc.SEAM_N), p, pc.seam_breaks(p, 0))))
    return out


# ---- the steps' blocks (tests/test_gpu_mixed_steps.py) ------------------------------------------

def run_and_stretch(p, run, stretch, seed=0, noise=3000):
    """Noise, a stretch of `stretch` bytes of a primitive unit of period p, noise, a run of `run` zeros, noise."""
    return pc.cat(pc.filler(noise, seed), pc.stretch(p, stretch, seed), pc.filler(noise, seed + 1), np.zeros(run, np.uint8),
                  pc.filler(noise, seed + 2))


def inner_run_unit(p, inner, seed=0):
    """A unit of p bytes that begins with a run of `inner` equal bytes (1 <= inner < p); its last byte occurs once."""
    u = pc.unit(p, seed)
    u[:inner] = 100
    if inner < p - 1 and u[inner] == 100:
        u[inner] = 101
    return u


def short_runs_beside_stretches(p, lo, seed=0):
    """Stretches of period p, with runs of lo ... p - 1 equal bytes between them (runs the run step ranks and the period
    step's lengths forget), a long run of zeros, and a stretch of a unit a...ab whose inner run is lo bytes or more."""
    rng = np.random.default_rng([41, p, seed])
    parts = [pc.filler(1000, seed)]
    for i in range(6):
        parts += [pc.stretch(p, 9000 + 17 * i, seed), np.full(int(rng.integers(lo, p)), 30 + i, np.uint8), pc.filler(50, 50 + i)]
    parts += [np.zeros(8192, np.uint8), pc.filler(100, 70)]
    inner = max(lo, min(p - 1, (lo + p) // 2))
    parts += [np.tile(inner_run_unit(p, inner, seed), 40000 // p + 1), pc.filler(100, 71)]
    return pc.cat(*parts)


def seam_blocks(p, L=20000):
    """(name, block): a run that ends where a stretch begins with the run's byte, and a stretch that ends in a run of its
    last byte; each with the byte behind it below and above what would go on."""
    u = pc.unit(p, 0)
    S = pc.stretch(p, L)
    out = []
    for name, low in (("falling", True), ("rising", False)):
        end = [1] if low else [252]
        out.append(("a run into a stretch, " + name, pc.cat(pc.filler(500, 1), np.full(6000, u[0], np.uint8), S, end, pc.filler(500, 2),
                                                              np.full(5000, u[0], np.uint8), S[:L // 2], end, pc.filler(100, 3))))
        out.append(("a stretch into a run, " + name, pc.cat(pc.filler(500, 4), S, np.full(6000, S[-1], np.uint8), end, pc.filler(500, 5),
                                                              S[:L // 2 + L % p], np.full(7000, S[-1], np.uint8), end, pc.filler(100, 6))))
    return out


def plain_blocks():
    """(name, block): nothing mixed -- the switch must change nothing."""
    from bwtc_amd import synth
    rng = np.random.default_rng(5)
    one_run = rng.integers(1, 256, 300000).astype(np.uint8)
    one_run[100000:100000 + (1 << 16)] = 0
    return [("zeros", np.zeros(300000, np.uint8)), ("one run in noise", one_run), ("one stretch without runs", pc.stretch(9, 1 << 18)),
            ("random bytes", rng.integers(0, 256, 300000).astype(np.uint8)), ("generator text", synth.gen_text(1 << 20, 3))]


RANDOM_PERIODS = (2, 3, 5, 9, 16, 17, 64, 100, 257)


def random_block(it):
    """Block `it` of the randomised case -> (block, starting points, p): a run of 4096 bytes or more, ONE stretch of 2^15
    bytes or more of a primitive unit of period p, further runs and short stretches of that period, and noise."""
    rng = np.random.default_rng([20260101, it])
    p = int(RANDOM_PERIODS[it % len(RANDOM_PERIODS)])
    parts = [np.full(int(rng.integers(4096, 20000)), rng.integers(0, 256), np.uint8),
             pc.stretch(p, int(rng.integers(1 << 15, 3 << 15)), it % 2, int(rng.integers(0, p)))]
    for _ in range(int(rng.integers(2, 10))):
        kind = rng.random()
        if kind < 0.3:
            parts.append(np.full(int(rng.integers(1, 3000)), rng.integers(0, 256), np.uint8))
        elif kind < 0.6:
            parts.append(pc.stretch(p, int(rng.integers(p, 40 * p)), it % 2, int(rng.integers(0, p))))
        else:
            parts.append(pc.filler(int(rng.integers(1, 3000)), int(rng.integers(0, 100))))
    order = rng.permutation(len(parts))
    sep = [pc.filler(int(rng.integers(1, 30)), 200 + i) for i in range(len(parts))]
    d = pc.cat(*[x for i in order for x in (parts[i], sep[i])])
    return d, (1, 8)[it % 2], p


# ---- premises -----------------------------------------------------------------------------------

def votes_np(T, depth):
    """periodmodel.votes() with numpy: {distance: votes} over the list sorted to `depth` characters."""
    T = np.asarray(T, np.uint8)
    rank = mixedmodel._rank_by(T, depth, {})
    order = np.lexsort((-np.arange(T.size), rank))
    same = rank[order[1:]] == rank[order[:-1]]
    d = np.abs(order[1:] - order[:-1])[same]
    d = d[(d >= 2) & (d <= PERIOD_MAX)]
    return dict(zip(*[x.tolist() for x in np.unique(d, return_counts=True)])) if d.size else {}


def facts(T, p):
    """(the longest run, the longest proper stretch of period p) of T."""
    T = np.asarray(T, np.uint8)
    return period_lengths_np(T, 1)[1], mixedmodel.longest_proper_np(T, p)
