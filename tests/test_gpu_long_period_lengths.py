"""The stretch-length pass at periods above 4096 on the GPU (-m gpu), through the hook bwtc_hip_test_long_period_lengths:
the product's own stretch_lengths with both maxima, held to tests/longperiodmodel.py lengths() by exact equality, with
breaks one before, on and one behind a load's, a thread's, a wave's and a tile's seam (tests/longcases.py seams()).
Without the long periods the hook does not exist."""
import numpy as np
import pytest

import longcases as lc
import longperiodmodel as lm
import periodcases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from bwtc_amd import hip
    c = hip.Context(0, lc.LENGTHS_N)
    yield c
    c.close()


def _same(ctx, T, p):
    k, longest, proper = ctx.test_long_period_lengths(T, p)
    want_k, want_longest, want_proper = lm.lengths(T, p)
    assert (k == want_k).all(), (p, T.size, np.flatnonzero(k != want_k)[:8])
    assert (longest, proper) == (want_longest, want_proper), (p, T.size, longest, proper, want_longest, want_proper)
    return longest, proper


@pytest.mark.parametrize("p", lc.LENGTH_PERIODS)
def test_breaks_around_the_seams(ctx, p):
    for delta in (-1, 0, 1):
        T, at = lc.seam_block(p, delta)
        assert len(at) >= 5
        longest, _ = _same(ctx, T, p)
        assert longest < T.size


@pytest.mark.parametrize("p", lc.LENGTH_PERIODS)
def test_short_blocks_and_p_next_to_n(ctx, p):
    """p = n - 1 (one position can be a break), n = p + 2, a block that ends a byte behind a tile, and breaks exactly p
    before the seams (the first break at or behind s + p is looked for across the seam)."""
    for n in (p + 1, p + 2, (p // lc.TILE + 2) * lc.TILE + 1):
        T = pc.stretch(p, n)
        assert _same(ctx, T, p)[0] == n
        T[-1] ^= 1
        assert _same(ctx, T, p)[0] == n - 1
    n = min(lc.LENGTHS_N, 3 * p + 5 * lc.TILE)
    T = pc.with_breaks(pc.stretch(p, n), p, [q - p for q in lc.seams(p, n).values() if q - p >= p] + [n - 1])
    _same(ctx, T, p)
    T = lc.noise(n, p)                                             # nothing periodic: every position a break
    T[n // 2:n // 2 + 70] = 7                                      # ... and a run, which is no proper stretch
    _same(ctx, T, p)


def test_refusals_and_a_reused_context(ctx):
    """Large, tiny, refused, large on one context; a refusal leaves k_out as it was."""
    from bwtc_amd import hip
    big = lc.seam_block(16385, 0)[0]
    _same(ctx, big, 16385)
    tiny = pc.stretch(4097, 4098)
    _same(ctx, tiny, 4097)
    for T, p in ((tiny, 4096), (tiny, 1), (tiny, 0), (tiny, 4098), (tiny, 5000), (big, (1 << 24) + 1), (np.zeros(lc.LENGTHS_N + 2, np.uint8), 5000)):
        k_out = np.full(max(T.size, 1), 0x5A5A5A5A, np.uint32)
        with pytest.raises(hip.BwtcHipError):
            ctx.test_long_period_lengths(T, p, k_out)
        assert (k_out == 0x5A5A5A5A).all(), p
    with pytest.raises(hip.BwtcHipError):
        ctx.test_period_lengths(tiny, 4097)                        # the short hook keeps its limit
    _same(ctx, big, 16385)
