"""Test-side model of the inverse transform (bwtc_amd/csrc/inverse_bwt.hip), the part tests/hrecord.py,
tests/pgrammar.py and tests/wforest.py play for their stages: plain numpy, nothing of bwtc_amd.

The row model is the one in the header comment of inverse_bwt.hip: N = size + 1 rows, L[i] = bwt[i] for i < size,
L[size] = bwt[eob], eob = lf[0]; LF is ONE stable sort of the rows other than eob (LF = 1 + place in that order),
LF(eob) = 0; the block is out[i] = L[LF^i(0)].  From the walk the model gives the exact outcome of ANY input, damaged
or not: the bytes, or the return code.  Also here: blocks with a chosen end-of-block row, the blocks both test
files of the inverse share, and controlled damage (two cycles, a cycle without a splitter row, one cycle again)."""
import collections

import numpy as np

SPLIT = 64                                  # kSplit: one splitter row per 64 rows
SIZES = (1, 2, 62, 63, 64, 127, 128, 510, 511, 512, 4094, 4095, 4096, 8191, 65534, 65535, 65536, (1 << 20) + 3)
N_LFS = (1, 2, 3, 7, 8, 255, 256)
DAMAGE_SIZES = (300, 4096, 65536)

Model = collections.namedtuple("Model", "rc out walk pos one_cycle powers_ok LF L")


def block_with_eob(size, eob, rng, sigma=256):
    """A block whose end-of-block row is exactly eob (1 <= eob <= size): the last byte is 128 and occurs nowhere
    else, exactly eob - 1 of the others are below 128.  (The transform sorts the REVERSED block followed by a zero
    byte; the row of the whole string is the number of suffixes that start below 128: those eob - 1 and the zero.)"""
    assert 1 <= eob <= size
    half = max(1, min(127, sigma // 2))
    b = (129 + rng.integers(0, half, size)).astype(np.uint8)
    low = rng.permutation(size - 1)[:eob - 1]
    b[low] = rng.integers(0, half, eob - 1)
    b[size - 1] = 128
    assert int((b < 128).sum()) == eob - 1 and int((b == 128).sum()) == 1
    return b


def eobs(size):
    return sorted({e for e in (1, 63, 64, 65, 511, 512, 4095, 4096, size - 1, size) if 1 <= e <= size})


def block_names(size):
    return ["random256", "random2", "all_equal"] + ["eob_%d" % e for e in eobs(size)]


def block(size, name):
    """The blocks both test files use, by name; the same bytes every time."""
    kinds = block_names(size)
    rng = np.random.default_rng(1000003 * kinds.index(name) + size)
    if name == "random256":
        return rng.integers(0, 256, size).astype(np.uint8)
    if name == "random2":
        return (rng.integers(0, 2, size) * 7 + 97).astype(np.uint8)
    if name == "all_equal":
        return np.full(size, 0x5A, np.uint8)
    return block_with_eob(size, int(name[4:]), rng, sigma=(256, 4, 16)[size % 3])


def starting_points(size, name):
    """Starting points of a shared block: every count of N_LFS in turn (the oracle gives one power up to 256 bytes)."""
    return N_LFS[(block_names(size).index(name) + SIZES.index(size)) % len(N_LFS)] if size in SIZES else 8


POWER_SIZES = (298, 4098, 65538)            # N = 299, 4099, 65539: no count of N_LFS above 1 divides them
OFF_BY_ONE = ((298, 256), (298, 8), (65538, 8), (4098, 256))


def power_blocks(size):
    """[(starting points, block)] for every count of N_LFS, end-of-block rows drawn."""
    rng = np.random.default_rng(size)
    return [(n_lf, block_with_eob(size, 1 + int(rng.integers(0, size)), rng, sigma=int(rng.choice([2, 256])))) for n_lf in N_LFS]


def plain_block(size, n_lf):
    return np.random.default_rng(size + n_lf).integers(0, 256, size).astype(np.uint8)


# ---- the row model ---------------------------------------------------------------------------------------------
def lf_table(bwt, eob):
    bwt = np.asarray(bwt, np.uint8)
    size = bwt.size
    L = np.zeros(size + 1, np.uint8)
    L[:size] = bwt
    if eob < size:
        L[size] = bwt[eob]                      # eob == size: the row's own character, never emitted
    rows = np.delete(np.arange(size + 1, dtype=np.int64), eob)
    order = np.argsort(L[rows], kind="stable")
    LF = np.zeros(size + 1, np.int64)
    LF[rows[order]] = 1 + np.arange(size, dtype=np.int64)
    return L, LF


def walk_from_zero(LF):
    """walk[i] = LF^i(0), i < N, by pointer doubling."""
    n = LF.size
    walk = np.zeros(n, np.int64)
    P, m = LF, 1
    while m < n:
        k = min(m, n - m)
        walk[m:m + k] = P[walk[:k]]
        P = P[P]
        m *= 2
    return walk


def cycle_labels(LF):
    """label[row] = smallest row of the row's cycle."""
    n = LF.size
    label, P, m = np.arange(n, dtype=np.int64), LF, 1
    while m < n:
        label = np.minimum(label, label[P])
        P = P[P]
        m *= 2
    return label


def cycles_without_splitter(LF):
    """Number of cycles of LF, and how many of them hold no splitter row (no multiple of 64)."""
    label = cycle_labels(LF)
    every = np.unique(label)
    with_split = np.unique(label[::SPLIT])
    return every.size, every.size - with_split.size


def lf_model(bwt, lf):
    """What the inverse must do with (bwt, lf): Model.rc is 0 (Model.out are the bytes), -1 (arguments) or -4 (LF is
    not one cycle of all N rows, or a power lf[k], k >= 1, is not at index k * (N / n_lf) - 1 of the walk from row 0).
    walk, pos (row -> first index on the walk, -1 off it), one_cycle and powers_ok (k >= 1) say why."""
    bwt = np.asarray(bwt, np.uint8)
    lf = [int(v) for v in lf]
    size, n_lf = bwt.size, len(lf)
    n = size + 1
    none = Model(-1, None, None, None, False, None, None, None)
    if n_lf == 0 or n_lf > 256:
        return none
    if size == 0:
        return none._replace(rc=0, out=bwt.copy())
    if lf[0] > size:
        return none
    if any(v > size for v in lf[1:]):
        return none._replace(rc=-4)
    L, LF = lf_table(bwt, lf[0])
    walk = walk_from_zero(LF)
    pos = np.full(n, -1, np.int64)
    pos[walk[::-1]] = np.arange(n - 1, -1, -1)
    one_cycle = bool((pos >= 0).all())
    x = n // n_lf
    powers_ok = np.array([pos[lf[k]] == k * x - 1 for k in range(1, n_lf)], bool)
    rc = 0 if one_cycle and powers_ok.all() else -4
    return Model(rc, L[walk[:size]], walk, pos, one_cycle, powers_ok, LF, L)


def powers_after_last_splitter(model, lf):
    """The k >= 1 whose row lies after the last splitter row of the walk: its way on to a splitter ends at row 0."""
    last = int(model.pos[::SPLIT].max())
    return [k for k in range(1, len(lf)) if model.pos[int(lf[k])] > last]


def wrap_case(transform, size=257, sp=256, seeds=range(64)):
    """The first seed whose block has LF powers after the last splitter row: (block, bwt, lf, those k).  transform is
    the oracle's forward transform, (block, starting points) -> (bwt, lf); with 258 rows and 256 powers x = 1, so
    the rows at walk indices 0..254 are all powers, and the end-of-block row (index 257) is kept off the splitters."""
    for seed in seeds:
        rng = np.random.default_rng(seed)
        eob = 1 + int(rng.integers(0, size))
        if eob % SPLIT == 0:
            continue
        d = block_with_eob(size, eob, rng)
        bwt, lf = transform(d, sp)
        ks = powers_after_last_splitter(lf_model(bwt, lf), lf)
        if len(ks) >= 2:
            return d, bwt, lf, ks
    raise AssertionError("no seed puts an LF power after the last splitter row")


# ---- controlled damage -------------------------------------------------------------------------------------------
# Swapping two neighbouring rows i, i + 1 with different characters (neither the end-of-block row, i + 1 < size)
# leaves every other row's LF alone and exchanges LF(i) and LF(i + 1): LF composed with one transposition, which
# splits a cycle in two when both rows lie on it and joins two cycles otherwise.
def _swappable(bwt, eob):
    i = np.arange(bwt.size - 1)
    return i[(bwt[:-1] != bwt[1:]) & (i != eob) & (i + 1 != eob)]


def swap(bwt, i):
    out = np.array(bwt, np.uint8, copy=True)
    out[i], out[i + 1] = bwt[i + 1], bwt[i]
    return out


def damage_two_cycles(bwt, lf):
    """One swap -> exactly two cycles, both with splitter rows where the block allows: the swap whose rows are
    farthest apart on the walk."""
    m = lf_model(bwt, lf[:1])
    assert m.one_cycle
    cand = _swappable(bwt, int(lf[0]))
    gap = np.abs(m.pos[cand] - m.pos[cand + 1])
    return swap(bwt, int(cand[np.argmax(np.minimum(gap, bwt.size + 1 - gap))]))


def damage_cycle_without_splitter(bwt, lf):
    """One swap whose split-off cycle holds no splitter row: rows walk[a + 1 .. b] with a, b the two rows' places."""
    m = lf_model(bwt, lf[:1])
    assert m.one_cycle
    cand = _swappable(bwt, int(lf[0]))
    a, b = np.minimum(m.pos[cand], m.pos[cand + 1]), np.maximum(m.pos[cand], m.pos[cand + 1])
    for j in np.argsort(b - a, kind="stable"):
        if (m.walk[a[j] + 1:b[j] + 1] % SPLIT != 0).all():
            return swap(bwt, int(cand[j]))
    raise AssertionError("no swap splits off a cycle without a splitter row")


def damage_one_cycle(bwt, lf):
    """Two swaps: the first splits the cycle, the second joins the halves again.  Four bytes differ, LF is one cycle
    of all rows, and with a single LF power there is nothing left to refuse: the bytes are the model's."""
    first = damage_two_cycles(bwt, lf)
    eob = int(lf[0])
    label = cycle_labels(lf_table(first, eob)[1])
    cand = _swappable(first, eob)
    untouched = (first[cand] == bwt[cand]) & (first[cand + 1] == bwt[cand + 1])
    joins = cand[(label[cand] != label[cand + 1]) & untouched]
    assert joins.size, "no second swap joins the two cycles"
    return swap(first, int(joins[0]))
