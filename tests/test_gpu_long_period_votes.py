"""The long finder on the GPU (-m gpu), through the hook bwtc_hip_test_long_period_votes: sweep 1 (the vote kernel with
the coarse table), the pick of the coarse bins, sweep 2 (the fine tables) and the merged candidates over given lists,
held to tests/longperiodmodel.py candidates() by exact equality -- distances, votes, order, the zeros behind the last
candidate and the guard words behind the 16 the hook writes.  Without the long finder the hook does not exist."""
import numpy as np
import pytest

import longcases as lc
import longperiodmodel as lm

pytestmark = pytest.mark.gpu

CAP = (1 << 24) + (1 << 16)
KMASK = (1 << 56) - 1
GUARD = 0xABCD1234


@pytest.fixture(scope="module")
def ctx():
    from bwtc_amd import hip
    c = hip.Context(0, CAP)
    yield c
    c.close()


def _zig(spec, base=5):
    """One group per (distance, votes): its members alternate between two positions d apart, so every neighbouring pair
    votes for d and no position passes 2^24 + base + 1.  The keys' upper byte differs inside a group (kmask hides it)."""
    ks, vs = [], []
    for g, (d, votes) in enumerate(spec):
        for i in range(votes + 1):
            vs.append(base + g + (d if i % 2 else 0))
            ks.append(g | ((i % 3) << 56))
    return np.array(ks, np.uint64), np.array(vs, np.uint32)


def _check(ctx, ks, vs, need, k1=None, kmask=KMASK):
    got, out = ctx.test_long_period_votes(ks, vs, kmask, need, k1)
    want = lm.candidates((ks, vs), kmask, need, k1)
    assert got == want, (got, want)
    assert not out[2 * len(got):16].any() and (out[16:] == GUARD).all(), out
    return got


def test_the_ends_of_the_range(ctx):
    """4096 is the short table's, 4097 and 2^24 the long finder's, 2^24 + 1 nobody's."""
    got = _check(ctx, *_zig([(4096, 300), (4097, 301), (1 << 24, 302), ((1 << 24) + 1, 400)]), 256)
    assert got == [(1 << 24, 302), (4097, 301), (4096, 300)]
    assert _check(ctx, *_zig([((1 << 24) + 1, 400), (1, 500)]), 256) == []


@pytest.mark.parametrize("d", [8191, 12287])
def test_coarse_bin_seams(ctx, d):
    """d and d + 1 on either side of a coarse bin's seam; each alone, and both."""
    assert _check(ctx, *_zig([(d, 300), (d + 1, 299)]), 256) == [(d, 300), (d + 1, 299)]
    assert _check(ctx, *_zig([(d, 300), (d + 1, 200)]), 256) == [(d, 300)]
    assert _check(ctx, *_zig([(d, 200), (d + 1, 300)]), 256) == [(d + 1, 300)]
    # neither has `need` votes, their coarse bins together would: nothing
    assert _check(ctx, *_zig([(d, 200), (d + 1, 200)]), 256) == []


def test_two_in_one_coarse_bin_and_the_threshold(ctx):
    assert _check(ctx, *_zig([(20000, 400), (20001, 500), (23000, 255), (23001, 256)]), 256) == [(20001, 500), (20000, 400), (23001, 256)]
    # a coarse bin that reaches `need` with two distances that do not: sweep 2 runs and finds nothing
    assert _check(ctx, *_zig([(30000, 255), (30002, 255)]), 256) == []
    assert _check(ctx, *_zig([(30000, 255)]), 256) == [] and _check(ctx, *_zig([(30000, 256)]), 256) == [(30000, 256)]


def test_more_than_eight_and_equal_votes(ctx):
    spec = [(70000 - 4500 * i, 300 + (i % 3)) for i in range(12)] + [(9, 301), (4096, 300)]
    got = _check(ctx, *_zig(spec), 256)
    assert len(got) == 8 and [v for _, v in got] == sorted((v for _, v in got), reverse=True)
    assert all(a[0] < b[0] for a, b in zip(got, got[1:]) if a[1] == b[1])          # the smaller distance first among equals


def test_short_and_long_together(ctx):
    got = _check(ctx, *_zig([(9, 1000), (5000, 900), (64, 800), (1 << 20, 1100), (4097, 256), (2, 255)]), 256)
    assert got == [(1 << 20, 1100), (9, 1000), (5000, 900), (64, 800), (4097, 256)]


def test_neighbours_of_different_groups_do_not_vote(ctx):
    """Every neighbouring pair lies 6000 apart; the pairs inside a group are 300, those across two groups 1200."""
    vs = np.array([7 + (6000 if i % 2 else 0) for i in range(1504)], np.uint32)
    ks = np.array([i // 5 for i in range(1504)], np.uint64)                 # groups of five: 4 pairs inside, 1 across
    inside = sum(1 for i in range(1503) if i // 5 == (i + 1) // 5)
    assert inside < 1503 and _check(ctx, ks, vs, 256) == [(6000, inside)]
    assert _check(ctx, ks, vs, inside + 1) == []
    # ... and with a mask that hides every key bit all of them are one group
    assert _check(ctx, ks, vs, 256, kmask=0) == [(6000, 1503)]


def _random_list(m, seed, cap=1 << 22):
    rng = np.random.default_rng([43, m, seed])
    dist = rng.choice([2, 9, 4096, 4097, 8191, 8192, 8193, 50000, 50001, 1 << 21, 3], m, p=[.05, .1, .1, .1, .1, .1, .05, .1, .1, .1, .1])
    vs = np.zeros(m, np.int64)
    for i in range(1, m):
        vs[i] = vs[i - 1] + dist[i] if vs[i - 1] + dist[i] < cap else vs[i - 1] - dist[i]
    vs = np.abs(vs)
    ks = np.cumsum(rng.random(m) < 0.05).astype(np.uint64) | (rng.integers(0, 200, m).astype(np.uint64) << np.uint64(56))
    return ks, vs.astype(np.uint32)


@pytest.mark.parametrize("m", [2, 16383, 16384, 16385, 3 * 16384 + 77, 65535, 65536, 65537, 3 * 65536 + 77])
def test_list_lengths_around_a_tile(ctx, m):
    """Lists of one entry less than a tile of 16 384 entries, a tile, one more and several tiles, and of 65 535 ... 65 537
    entries: a tile's count is a 16-bit half of an LDS word, and a list of 2^16 entries is four tiles, not one; the pair
    across a tile's seam votes once."""
    ks, vs = _random_list(m, 0)
    need = max(256, (m - 1) // 64 + 1)
    got = _check(ctx, ks, vs, need)
    assert m == 2 or len(got) >= 3, got
    if m > 16384:
        # the pair across the first tile's seam counts once: a list whose every pair votes for one distance, to the vote
        ks2, vs2 = np.zeros(m, np.uint64), np.where(np.arange(m) % 2, 9000, 0).astype(np.uint32)
        assert _check(ctx, ks2, vs2, need) == [(9000, m - 1)]


def test_a_list_in_window_order_votes_for_a_multiple(ctx):
    """The list of tests/longcases.py multiple_block(4100) with its groups' members by the suffix number's low 8 bits
    (longperiodmodel.window_order_list): the members of the stretch of period 4100 are neighbours 64 periods apart, and
    the winner is 262 400, a multiple of the period -- the list the division is for."""
    d = lc.multiple_block(4100)
    ks, vs = lm.window_order_list(d, 8)
    got = _check(ctx, ks, vs, lm.need_of(d.size))
    assert got and got[0][0] == lc.MULTIPLE_OF[4100] and not [c for c in got if c[0] <= 4100], got


def test_the_run_rule(ctx):
    """Two members of one run do not vote: k1[min(a, b)] > d, for short and long distances, at the seam d == k1."""
    ks, vs = _random_list(16000, 5)
    rng = np.random.default_rng(47)
    k1 = rng.choice([1, 4097, 8192, 8193, 50001, 1 << 22], 1 << 22).astype(np.uint32)
    with_rule = _check(ctx, ks, vs, 256, k1)
    without = _check(ctx, ks, vs, 256)
    assert with_rule != without and with_rule, (with_rule, without)
    assert _check(ctx, ks, vs, 256, np.zeros(1 << 22, np.uint32)) == without


def test_refusals(ctx):
    from bwtc_amd import hip
    ks, vs = _zig([(5000, 300)])
    for bad in (lambda: ctx.test_long_period_votes(ks, vs, KMASK, 0),                    # need == 0
                lambda: ctx.test_long_period_votes(ks, vs, KMASK, 4),                    # (m - 1) / need above 64
                lambda: ctx.test_long_period_votes(ks[:1], vs[:1], KMASK, 256),          # a list of one
                lambda: ctx.test_long_period_votes(ks, vs + np.uint32(CAP + (1 << 21)), KMASK, 256)):   # a suffix above the block size
        with pytest.raises(hip.BwtcHipError):
            bad()
    assert _check(ctx, ks, vs, 256) == [(5000, 300)]                                    # the context is as good as before
