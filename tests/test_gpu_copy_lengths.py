"""The copy round's three passes -- marks, flags, lengths (bwt_engine.hip, "Copies"; BWTC_HIP_COPIES=1) -- on the GPU
(-m gpu), through the hook bwtc_hip_test_copy_lengths: the sorter's launch code over a hand-made list and rank[], no text.
Every result is compared with copymodel.copy_lengths_np by exact equality of all n words and the maximum; the hook puts
canaries behind K[], the flags and the groups' marks and answers -20 - i where one changed.

The marks kernel takes 1024 entries per workgroup, entry tile * 1024 + row * 256 + thread: a wave's seams lie at every 64
entries, a workgroup's at every 1024.  The lengths' pass takes 64 positions per thread and 16 384 per tile.

Without the feature the hook does not exist."""
import numpy as np
import pytest

import copymodel as cm

pytestmark = pytest.mark.gpu

SIZE = (1 << 20) + 4096
SEAMS = (64, 128, 256, 1024, 2048, 3072)


@pytest.fixture(scope="module")
def ctx():
    from bwtc_amd import hip
    c = hip.Context(0, SIZE)
    yield c
    c.close()


def _list(n, groups, seed=0):
    """groups: [(suffixes, successor values)] in list order -- rank[s + 1] = the value given for member s (None: left as
    it is); every other rank is random.  -> (suf, grp, rank)."""
    rank = np.random.default_rng([89, n, seed]).integers(0, n, n).astype(np.uint32)
    suf, grp = [], []
    for g, (members, values) in enumerate(groups):
        for s, v in zip(members, values):
            suf.append(s)
            grp.append(g)
            if v is not None and s + 1 < n:
                rank[s + 1] = v
    return np.array(suf, np.uint32), np.array(grp, np.uint32), rank


def _check(ctx, suf, grp, rank, what):
    n = rank.size
    want, longest = cm.copy_lengths_np(suf, grp, rank, n)
    out = np.full(n + 64, 0xDEADBEEF, np.uint32)
    got, got_longest = ctx.test_copy_lengths(suf, grp, rank, out)
    assert (got == want).all(), (what, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
    assert got_longest == longest, (what, got_longest, longest)
    assert (out[n:] == 0xDEADBEEF).all(), what
    return want, longest


def _copies(L, c, lead=0, gap=5):
    """c copies of L positions, the first at position 0 and `gap` positions between them: group t holds the positions
    base + t, all good, so the flags' stretches are [base, base + L).  lead: a leading bad group of that many entries, which
    moves every later group by as many entries against the kernel's seams."""
    n = c * (L + gap) + lead + 3
    bases = [j * (L + gap) for j in range(c)]
    groups = []
    if lead:
        at = c * (L + gap)
        groups.append(([at + j for j in range(lead)], [7 + j for j in range(lead)]))
    groups += [([b + t for b in bases], [(t * 31 + 5) % n] * c) for t in range(L)]
    return n, groups, bases


@pytest.mark.parametrize("L", [63, 64, 65, 16383, 16384, 16385, 5 * 16384 + 17])
def test_stretches_of_flags(ctx, L):
    """Two and three copies of L positions, the first stretch from position 0: the stretches end at 63 / 64 / 65 and at
    16 383 / 16 384 / 16 385 positions and run across several tiles' carry; K counts down from L in each copy.  With a
    leading group of 1 or 3 entries the groups of two and three straddle the waves' and workgroups' seams."""
    for c, lead in ((2, 0), (2, 1), (3, 0), (3, 1), (2, 3)):
        n, groups, bases = _copies(L, c, lead)
        suf, grp, rank = _list(n, groups, L)
        want, longest = _check(ctx, suf, grp, rank, (L, c, lead))
        assert longest == L and all(want[b] == L and want[b + L - 1] == 1 and want[b + L] == 0 for b in bases), (L, c, lead)


@pytest.mark.parametrize("seam", SEAMS)
def test_the_only_disagreeing_pair_on_a_seam(ctx, seam):
    """A group of four entries seam - 2 ... seam + 1 whose only disagreeing neighbours are the entries seam - 1 and seam; a
    group of two at seam - 1, seam that disagrees, and one that agrees.  Everything before and behind agrees."""
    for size, differ in ((4, True), (2, True), (2, False), (4, False)):
        first = seam - size // 2                          # the seam group's first entry
        n = 4 * seam + 64
        groups, s = [], 0
        while s + 2 <= first - 2 or (s < first and first - s in (2, 3)):
            k = first - s if first - s in (2, 3) else 2
            groups.append((list(range(s, s + k)), [11] * k))
            s += k
        assert s == first, (seam, size, s, first)
        members = list(range(2 * seam, 2 * seam + size))  # positions of their own, side by side: K chains where they are good
        values = [21] * (size // 2) + [22 if differ else 21] * (size // 2)
        groups.append((members, values))
        groups.append(([3 * seam, 3 * seam + 2], [31, 31]))
        suf, grp, rank = _list(n, groups, seam)
        want, _ = _check(ctx, suf, grp, rank, (seam, size, differ))
        assert suf.size > seam and grp[seam - 1] == grp[seam] == len(groups) - 2
        assert (want[members] == 0).all() if differ else (want[members] > 0).all(), (seam, size, differ, want[members])
        assert want[3 * seam] == 1 and want[0] > 0


def test_first_and_last_entry_and_the_block_end(ctx):
    """The disagreeing pair at entries 0, 1 and at m - 2, m - 1; a member with s + 1 = n; lists of one group."""
    n = 5000
    mid = [([100 + 2 * g, 101 + 2 * g], [g, g]) for g in range(700)]
    for what, groups in (("first", [([10, 20], [1, 2])] + mid), ("last", mid + [([10, 20], [1, 2])]),
                         ("both", [([10, 20], [1, 2])] + mid + [([30, 40, 50], [3, 3, 4])]),
                         ("the end is a member", mid + [([n - 1, 60], [None, 5])]),
                         ("the end and its predecessor", mid + [([n - 2, n - 1], [9, None])]),
                         ("one good group", [([10, 20, 30], [1, 1, 1])]), ("one bad group", [([10, 20, 30], [1, 1, 2])])):
        suf, grp, rank = _list(n, groups, len(what))
        want, _ = _check(ctx, suf, grp, rank, what)
        assert want[n - 1] == 0 and want[10] == (1 if what == "one good group" else 0), what
        if what == "the end and its predecessor":
            assert want[n - 2] == 0


def test_successors_in_two_groups_and_in_a_larger_one(ctx):
    """Successors in two groups of equal size: F is false.  Successors inside a larger group: F is true and K chains
    through it."""
    n = 400
    # G = {10, 20}; X = {11, 50}, Y = {21, 60}: two groups of two -- rank[11] != rank[21]
    two = [([10, 20], [100, 200]), ([11, 50], [7, 7]), ([21, 60], [8, 8])]
    suf, grp, rank = _list(n, two)
    want, _ = _check(ctx, suf, grp, rank, "two groups")
    assert want[10] == 0 and want[20] == 0 and want[11] == 1 and want[21] == 1
    # G = {10, 20}; H = {11, 21, 70}, all of whose successors lie in one group again; then nothing
    larger = [([10, 20], [100, 100]), ([11, 21, 70], [9, 9, 9]), ([12, 22, 71, 90], [1, 1, 1, 2])]
    suf, grp, rank = _list(n, larger)
    want, longest = _check(ctx, suf, grp, rank, "a larger group")
    assert want[10] == 2 and want[20] == 2 and want[11] == 1 and want[70] == 1 and want[12] == 0 and longest == 2


def _random_list(n, seed, p_bad):
    """Positions in stretches, dealt to groups of 1 ... 130 entries in a random order; a bad group has one disagreeing
    pair of neighbours."""
    rng = np.random.default_rng([97, n, seed])
    take = np.zeros(n, bool)
    at = 0
    while at < n:
        length = int(rng.integers(1, min(400, n // 8 + 2)))
        if at == 0 or rng.random() < 0.5:
            take[at:at + length] = True
        at += length
    S = rng.permutation(np.flatnonzero(take))
    groups, at = [], 0
    while at < S.size:
        k = min(int(rng.integers(1, 131)), S.size - at)
        values = [int(rng.integers(0, n))] * k
        if k >= 2 and rng.random() < p_bad:
            cut = int(rng.integers(1, k))
            values[cut:] = [(values[0] + 1) % n] * (k - cut)
        groups.append((S[at:at + k].tolist(), values))
        at += k
    return _list(n, groups, seed)


@pytest.mark.parametrize("n", [64, 16383, 16384, 16385, 3 * 16384 + 5])
def test_random_lists(ctx, n):
    """Every group bad, no group bad, and half of them, over positions in stretches."""
    for seed, p_bad in enumerate((1.0, 0.0, 0.5, 0.1)):
        suf, grp, rank = _random_list(n, seed, p_bad)
        want, longest = _check(ctx, suf, grp, rank, (n, p_bad))
        if p_bad == 1.0:
            sizes = np.bincount(grp)
            assert (want[suf[sizes[grp] > 1]] == 0).all()
        if p_bad == 0.0:
            ends = grp[suf == n - 1]                       # (the group that holds n - 1, if any, fails F)
            assert longest > 0 and (want[suf[~np.isin(grp, ends)]] > 0).all()


def test_tiny_and_large(ctx):
    """n = 1 and 2, and a list over 2^20 + 3 positions."""
    for suf, grp, rank in (([0], [0], [0]), ([0, 1], [0, 0], [1, 1]), ([0], [0], [1, 0]), ([1], [0], [0, 1]), ([1, 0], [0, 1], [0, 0])):
        _check(ctx, np.array(suf, np.uint32), np.array(grp, np.uint32), np.array(rank, np.uint32), (suf, grp, rank))
    suf, grp, rank = _random_list((1 << 20) + 3, 5, 0.2)
    _, longest = _check(ctx, suf, grp, rank, "2^20 + 3")
    assert longest > 1


def test_refusals_and_reuse(monkeypatch):
    """One context: large, tiny, refused (nothing is written), large again."""
    from bwtc_amd import hip
    monkeypatch.setenv("BWTC_HIP_COPIES", "1")
    c = hip.Context(0, 1 << 20)
    monkeypatch.delenv("BWTC_HIP_COPIES")
    try:
        large = _random_list(200000, 1, 0.3)
        tiny = (np.array([0, 2], np.uint32), np.array([0, 0], np.uint32), np.array([0, 3, 1, 3], np.uint32))
        _check(c, *large, "large")
        _check(c, *tiny, "tiny")
        suf, grp, rank = tiny
        bad = [(suf[:0], grp[:0], rank), (suf, grp, rank[:0]), (suf, grp, np.zeros((1 << 20) + 1, np.uint32)),
               (np.array([0, 4], np.uint32), grp, rank), (suf, np.array([0, 2], np.uint32), rank), (suf, np.array([1, 1], np.uint32), rank),
               (np.array([2, 2], np.uint32), grp, rank)]
        for a, b, r in bad:
            out = np.full(max(r.size, 4), 0xDEADBEEF, np.uint32)
            with pytest.raises(hip.BwtcHipError) as e:
                c.test_copy_lengths(a, b, r, out)
            assert e.value.code == -1 and (out == 0xDEADBEEF).all(), (a, b, r.size)
        _check(c, *large, "large again")
    finally:
        c.close()
