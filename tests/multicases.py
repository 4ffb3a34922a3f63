"""The blocks of the several-period steps' tests (tests/test_gpu_period_merge.py, tests/test_gpu_period_winners.py,
tests/test_gpu_multi_steps.py), built here so that tests/test_multimodel.py can prove, without a GPU, that every named
block has the edge it is named for.

The step blocks are written as the sorter's T; block() turns one into what a caller hands to bwt_block(), which sorts the
reverse.  A stretch reversed is a stretch of the same period and length."""
import numpy as np

import mixedcases as mc
import mixedmodel
import periodcases as pc
from periodmodel import PERIOD_MAX, period_lengths_np

TILE = pc.TILE


# ---- the model's texts (tests/test_multimodel.py) -------------------------------------------

MODEL_SETS = ((1, 2), (2, 3), (1, 2, 3), (2, 4), (4, 6), (3, 5), (1, 3, 4), (2, 3, 5), (1, 2, 3, 4), (3, 7, 10), (5, 6, 9))


def model_text(seed):
    """(text, periods): stretches of every period of a set (units a...ab included), runs, noise and copies of a shared
    tail behind stretches, over 2 ... 4 symbols, 40 ... 400 bytes."""
    rng = np.random.default_rng([43, seed])
    sigma = int(rng.integers(2, 5))
    periods = MODEL_SETS[seed % len(MODEL_SETS)]
    n = int(rng.integers(40, 401))
    units = {}
    for p in periods:
        u = rng.integers(0, sigma, p).astype(np.uint8)
        if p > 1 and rng.random() < 0.3:
            u[:] = u[0]
            u[-1] = (u[0] + 1) % sigma
        units[p] = u
    tail = rng.integers(0, sigma, int(rng.integers(2, 10))).astype(np.uint8)
    parts, have = [], 0
    while have < n:
        kind = rng.random()
        if kind < 0.15:
            q = np.full(int(rng.integers(1, 30)), rng.integers(0, sigma), np.uint8)
        elif kind < 0.75:
            p = int(periods[int(rng.integers(0, len(periods)))])
            q = np.tile(np.roll(units[p], -int(rng.integers(0, p))), 64 // p + 8)[:int(rng.integers(p, 8 * p + 12))]
            if rng.random() < 0.5:
                q = np.concatenate([q, tail])
        else:
            q = rng.integers(0, sigma, int(rng.integers(1, 10))).astype(np.uint8)
        parts.append(q)
        have += q.size
    return bytes((np.concatenate(parts)[:n] + 97).astype(np.uint8)), periods


# ---- the merging pass's blocks (tests/test_gpu_period_merge.py) ------------------------------

MERGE_SIZES = (1, 63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385, 2 * 16384 + 3, 5 * 16384 + 17)
MERGE_PERIODS = (1, 2, 3, 9, 64, 300, 4096)
MERGE_SEAMS = (64, 128, 4096, 8192, 16384, 2 * 16384, 4 * 16384)      # a thread's 64 positions, a wave's 4096, a tile's 16384


def merge_text(n, p, delta):
    """n bytes of period p with a break at seam + delta for every seam of the pass (those that can be breaks: p <= q < n)
    and one at n - 2 + delta."""
    S = pc.stretch(p, n)
    at = sorted({q + delta for q in MERGE_SEAMS + (n - 2,) if p <= q + delta < n})
    return pc.with_breaks(S, p, at) if at else S


def merge_olds(kp, seed):
    """(name, old words) for a step whose lengths are kp: never taken; taken by as long a stretch (the step takes it
    again); by one a character longer (kept); random lengths with stale member flags."""
    kp = np.asarray(kp, np.uint32)
    rng = np.random.default_rng([47, kp.size, seed & 0xFF])
    rand = rng.integers(0, 2 * int(kp.max()) + 3, kp.size).astype(np.uint32)
    rand[rng.random(kp.size) < 0.3] = 0
    rand |= (rng.random(kp.size) < 0.5).astype(np.uint32) << np.uint32(31)
    return [("all 0", np.zeros(kp.size, np.uint32)), ("equal to k_p", kp.copy()), ("k_p + 1", kp + np.uint32(1)), ("random", rand)]


def merge_depths(kp):
    """The step's depths: one below, at and one above the length of the suffix a third into the block."""
    k = int(kp[kp.size // 3])
    return sorted({max(1, k - 1), max(1, k), k + 1})


# ---- the finder's tables (tests/test_gpu_period_winners.py) ------------------------------------

def vote_tables(need):
    """(name, table of PERIOD_MAX + 1 votes) around a threshold `need` >= 8."""
    rng = np.random.default_rng([53, need])
    low = rng.integers(0, need, PERIOD_MAX + 1).astype(np.uint32)      # every bin below the threshold
    out = [("no bin over need", low.copy())]
    t = low.copy(); t[777] = need
    out.append(("one bin at need", t))
    t = low.copy(); t[[5, 9, 300, 12, 4000, 64, 2, 4096]] = need + np.arange(8, dtype=np.uint32) * 3
    out.append(("exactly 8", t))
    t = low.copy(); t[rng.choice(np.arange(2, PERIOD_MAX + 1), 40, replace=False)] = need + rng.permutation(40).astype(np.uint32)
    out.append(("more than 8", t))
    t = low.copy(); t[[3000, 17, 250, 18, 2, 4096, 1000, 999, 5, 6]] = need + 5
    out.append(("equal votes", t))
    t = low.copy(); t[[3000, 17]] = need + 9; t[[40, 4]] = need + 9; t[100] = need + 10
    out.append(("equal votes among different ones", t))
    t = np.zeros(PERIOD_MAX + 1, np.uint32); t[2] = need; t[4096] = need + 1
    out.append(("bins 2 and 4096", t))
    t = low.copy(); t[0] = 50 * need; t[1] = 60 * need; t[33] = need
    out.append(("votes in bins 0 and 1", t))
    t = np.full(PERIOD_MAX + 1, need, np.uint32)
    out.append(("every bin at need", t))
    t = np.zeros(PERIOD_MAX + 1, np.uint32); t[7] = 0xFFFFFFFF; t[8] = 0xFFFFFFFE
    out.append(("votes of 32 bits", t))
    return out


# ---- the steps' blocks (tests/test_gpu_multi_steps.py), as the sorter's T ------------------------

PAIRS = ((2, 3), (9, 12), (4, 6), (9, 300), (64, 300), (300, 9))
DIVISOR_PAIR = (3, 6)
# three planted periods -> the periods that take a step: 64 is a multiple of 2, which has more votes, and is skipped
TRIPLES = {(2, 9, 64): (2, 9), (5, 9, 64): (5, 9, 64)}


def block(T):
    """What bwt_block() is handed for the sorter to see T."""
    return np.ascontiguousarray(np.asarray(T, np.uint8)[::-1])


def stretches(periods, L, seed=0, noise=3000, run=0):
    """Noise, then for every period in turn a stretch of L bytes of a primitive unit and noise; run > 0: a run of that many
    zeros and noise at the end."""
    parts = [pc.filler(noise, seed)]
    for i, p in enumerate(periods):
        parts += [pc.stretch(p, L, seed + i), pc.filler(noise, seed + 1 + i)]
    if run:
        parts += [np.zeros(run, np.uint8), pc.filler(noise, seed + 9)]
    return pc.cat(*parts)


def merge_case(p=9, q=12, L=20000, copies=3, tail=48):
    """`copies` equal stretches of period p and as many of period q, each followed by the same `tail` bytes and then by
    noise of its own: the members of one step tie across the copies for k + tail characters, and find that out in one
    look-up at s + K -- if the later step leaves them their K."""
    same = pc.filler(tail, 77)
    parts = [pc.filler(500, 0)]
    for i in range(copies):
        parts += [pc.stretch(p, L), same, pc.filler(300, 10 + i)]
    for i in range(copies):
        parts += [pc.stretch(q, L, 1), same, pc.filler(300, 20 + i)]
    return pc.cat(*parts)


def seam_blocks(p, q, L=30000):
    """(name, T): stretches of two periods that run into each other and share bytes at the seam; falling and rising ends; a
    stretch that reaches the end of the text; a stretch that holds suffix 0."""
    A, B = pc.stretch(p, L), pc.stretch(q, L, 1)
    shared = pc.cat(A, B)
    shared[L:L + q] = np.resize(A[L - p:], q)             # the q-stretch begins with bytes that go on the p-stretch
    out = [("into each other", pc.cat(pc.filler(400, 1), A, B, pc.filler(400, 2), B[:L // 2], A[:L // 2], pc.filler(100, 3))),
           ("shared bytes at the seam", pc.cat(pc.filler(400, 4), shared, pc.filler(400, 5)))]
    for name, end in (("falling", 1), ("rising", 252)):
        out.append((name + " ends", pc.cat(pc.filler(300, 6), A, [end], pc.filler(300, 7), B, [end], pc.filler(300, 8), A[:L // 2], [end], B[:L // 2], [end])))
    out.append(("a stretch reaches the end", pc.cat(pc.filler(300, 9), A, pc.filler(300, 10), B)))
    out.append(("a stretch holds suffix 0", pc.cat(A, pc.filler(300, 11), B, pc.filler(300, 12))))
    return out


RANDOM_SETS = ((2, 3), (9, 12), (4, 6), (9, 300), (64, 300), (5, 17), (5, 9, 64), (3, 16, 100), (9, 257))


def random_block(it):
    """Block `it` of the randomised case -> (T, starting points, periods): one stretch of 2^15 bytes or more per period of
    a set no member of which divides another, further short stretches of those periods, runs (every third block holds one
    of 4096 bytes or more) and noise."""
    rng = np.random.default_rng([20260202, it])
    periods = RANDOM_SETS[it % len(RANDOM_SETS)]
    parts = [pc.stretch(p, int(rng.integers(1 << 15, 3 << 15)), it % 2, int(rng.integers(0, p))) for p in periods]
    if it % 3 == 0:
        parts.append(np.full(int(rng.integers(4096, 20000)), rng.integers(0, 256), np.uint8))
    for _ in range(int(rng.integers(2, 10))):
        kind = rng.random()
        if kind < 0.2:
            parts.append(np.full(int(rng.integers(1, 2000)), rng.integers(0, 256), np.uint8))
        elif kind < 0.6:
            p = int(periods[int(rng.integers(0, len(periods)))])
            parts.append(pc.stretch(p, int(rng.integers(p, 40 * p)), it % 2, int(rng.integers(0, p))))
        else:
            parts.append(pc.filler(int(rng.integers(1, 3000)), int(rng.integers(0, 100))))
    order = rng.permutation(len(parts))
    sep = [pc.filler(int(rng.integers(1, 30)), 200 + i) for i in range(len(parts))]
    return pc.cat(*[x for i in order for x in (parts[i], sep[i])]), (1, 8)[it % 2], periods


# ---- premises -----------------------------------------------------------------------------------

def facts(T, periods):
    """(the longest run, {p: the longest proper stretch of period p}) of T."""
    T = np.asarray(T, np.uint8)
    return period_lengths_np(T, 1)[1], {p: mixedmodel.longest_proper_np(T, p) for p in periods}


def vote_table(T, depth):
    """The finder's table over the list sorted to `depth` characters (mixedcases.votes_np) as PERIOD_MAX + 1 words."""
    t = np.zeros(PERIOD_MAX + 1, np.uint32)
    for d, v in mc.votes_np(T, depth).items():
        t[d] = v
    return t
