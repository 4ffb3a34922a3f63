"""The suffix sorter's period-length pass on the GPU (-m gpu), through the hook bwtc_hip_test_period_lengths: the
product's own three launches on the context's buffers, k_p[] and the longest stretch held to tests/periodmodel.py by
exact equality.  The blocks are tests/periodcases.py's; tests/test_periodmodel.py proves their premises -- where the
breaks lie -- without a GPU.

Without the feature the hook does not exist."""
import numpy as np
import pytest

import periodcases as pc
import periodmodel

pytestmark = pytest.mark.gpu

CAP = (1 << 20) + 4096


@pytest.fixture(scope="module")
def ctx():
    from bwtc_amd import hip
    c = hip.Context(0, CAP)
    yield c
    c.close()


def _same(ctx, T, p, what):
    want, longest = periodmodel.period_lengths_np(T, p)
    got, got_longest = ctx.test_period_lengths(T, p)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, p, T.size, "first difference at", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]), bad.size)
    assert got_longest == longest, (what, p, T.size, got_longest, longest)


@pytest.mark.parametrize("p", pc.PERIODS)
def test_lengths_of_every_size(ctx, p):
    """One stretch throughout (k = n - s everywhere) and random two-symbol text at every length: 1, p, p + 1, around a
    thread's 64 positions, a tile and two tiles, 17 tiles + 3 and 2^20 + 3; the lengths below p are blocks shorter
    than the period."""
    for n in pc.lengths_of(p):
        S = pc.stretch(max(p, 2), n) if p > 1 else np.full(n, 7, np.uint8)
        got, longest = ctx.test_period_lengths(S, p)
        assert (got == n - np.arange(n)).all() and longest == n, (p, n)
        _same(ctx, pc.two_symbols(n, p), p, "two symbols")


@pytest.mark.parametrize("p", pc.PERIODS)
def test_breaks_around_the_seams(ctx, p):
    """A break at -1 / 0 / +1 around a 16-byte load's, a thread's, a wave's and a tile's seam and the last position;
    a break exactly p before each seam; breaks p - 1, p and p + 1 apart."""
    q = max(p, 2)                                      # (the stretch's period; p = 1 sees it as noise with runs)
    S = pc.stretch(q, pc.SEAM_N)
    for delta in (-1, 0, 1):
        _same(ctx, pc.with_breaks(S, q, pc.seam_breaks(q, delta)), p, "seam %+d" % delta)
    _same(ctx, pc.with_breaks(S, q, pc.before_seam_breaks(q)), p, "p before the seams")
    _same(ctx, pc.with_breaks(S, q, pc.spaced_breaks(q)), p, "spaced breaks")
    if p > 1:
        flat = np.full(pc.SEAM_N, 9, np.uint8)          # a run is a stretch of every period
        flat[pc.SEAMS["wave"]] = 10
        _same(ctx, flat, p, "a run with one other byte")


def test_period_one_is_the_run_lengths(ctx):
    import runmodel
    rng = np.random.default_rng(1)
    T = np.repeat(rng.integers(0, 3, 4000).astype(np.uint8), rng.choice([1, 2, 3, 70, 300], 4000))
    k, longest = runmodel.run_lengths(bytes(T[:50000]))
    got, got_longest = ctx.test_period_lengths(T[:50000], 1)
    assert list(got) == k and got_longest == longest


def test_one_context_large_tiny_refused_large(ctx):
    from bwtc_amd import hip
    big = pc.with_breaks(pc.stretch(257, (1 << 20) + 3), 257, [5000, 700000])
    _same(ctx, big, 257, "large")
    _same(ctx, np.array([5, 5, 6], np.uint8), 2, "tiny")
    for T, p in ((big[:100], 0), (big[:100], 4097), (big[:0], 3), (np.zeros(CAP + (1 << 20), np.uint8), 3)):
        k_out = np.full(max(T.size, 4), 0xABCD1234, np.uint32)
        with pytest.raises(hip.BwtcHipError) as err:
            ctx.test_period_lengths(T, p, k_out)
        assert err.value.code == -1 and (k_out == 0xABCD1234).all(), (T.size, p)
    _same(ctx, big[::-1].copy(), 4096, "large again, another period")
    _same(ctx, big, 257, "large again")
