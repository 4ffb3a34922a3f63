"""The wide probe on the GPU (-m gpu), through the hook bwtc_hip_test_long_period_probe: one workgroup per window, held to
tests/longperiodmodel.py probe().  A window is clean when none of its `span` positions is a break of period p; the
windows are the aligned ones, p + i span, that end at or below n.  Without the long periods the hook does not exist."""
import numpy as np
import pytest

import longcases as lc
import longperiodmodel as lm
import periodcases as pc

pytestmark = pytest.mark.gpu

CAP = (1 << 24) + (1 << 18)


@pytest.fixture(scope="module")
def ctx():
    from bwtc_amd import hip
    c = hip.Context(0, CAP)
    yield c
    c.close()


def _planted(n, p, lo, hi, seed=0):
    """Noise with breaks everywhere but in [lo, hi): there T[q] == T[q - p]."""
    T = lc.noise(n, seed).copy()

    def disagree(start):                                           # p positions at a time: each sees its final predecessors
        for a in range(start, n, p):
            b = min(a + p, n)
            same = T[a:b] == T[a - p:b - p]
            T[a:b][same] += 1

    disagree(p)
    for a in range(lo, hi, p):
        b = min(a + p, hi)
        T[a:b] = T[a - p:b - p]
    disagree(hi)
    brk = lm.breaks_of(T, p)
    assert not brk[lo:hi].any() and brk[p:lo].all() and brk[hi:].all()
    return T


def _ask(ctx, T, p, span):
    got = ctx.test_long_period_probe(T, p, span)
    assert got == lm.probe(T, p, span), (p, span, got)
    return got


@pytest.mark.parametrize("span", [777, 14339, 16384, 16385, 40000])
def test_a_clean_stretch_around_an_aligned_window(ctx, span):
    """Spans below a turn of 256 x 64 positions, of one turn, of one and a bit, of several."""
    p, i = 4097, 3
    n = p + 6 * span + 11
    lo = p + i * span
    assert _ask(ctx, _planted(n, p, lo, lo + span), p, span)                  # exactly the window
    assert not _ask(ctx, _planted(n, p, lo, lo + span - 1), p, span)          # one byte short of it
    assert not _ask(ctx, _planted(n, p, lo + 1, lo + span), p, span)          # ... at its front
    assert not _ask(ctx, _planted(n, p, lo + 1, lo + span + 1), p, span)      # as long, one position off
    assert _ask(ctx, _planted(n, p, lo - 5, lo + span + 5), p, span)


def test_the_last_window_and_none(ctx):
    p, span = 5000, 20000
    n = p + 5 * span
    assert _ask(ctx, _planted(n, p, p + 4 * span, n), p, span)                # the only clean window ends at n
    assert not _ask(ctx, _planted(n + span - 1, p, p + 5 * span, n + span - 1), p, span)   # a clean tail that is no whole window
    assert _ask(ctx, _planted(n, p, p, p + span), p, span)                    # the first window: the chunk that holds position p
    assert not _ask(ctx, lc.noise(n, 4), p, span)
    assert not _ask(ctx, lc.noise(p + span, 5), p, span) and not _ask(ctx, lc.noise(100, 5), p, span)   # no window at all
    assert _ask(ctx, pc.stretch(p, n), p, span)


def test_both_ends_of_the_range(ctx):
    from bwtc_amd import hip
    span = 30000
    for p in (4097, 1 << 24):
        n = p + 3 * span + 7
        T = pc.stretch(9973, n)                                    # period 9973 is none of p
        for a in range(p + span, p + 2 * span, p):                 # ... but for the middle window (p positions at a time)
            b = min(a + p, p + 2 * span)
            T[a:b] = T[a - p:b - p]
        assert lm.probe(T, p, span) and _ask(ctx, T, p, span)
        T[p + span + 12345] ^= 1
        assert not _ask(ctx, T, p, span)
    T = pc.stretch(4097, 100000)
    for p, s in ((4096, 1000), ((1 << 24) + 1, 1000), (5000, 0)):
        with pytest.raises(hip.BwtcHipError):
            ctx.test_long_period_probe(T, p, s)
