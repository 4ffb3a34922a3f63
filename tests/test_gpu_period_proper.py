"""The stretch-length pass with its second maximum on the GPU (-m gpu), through the hook bwtc_hip_test_period_proper: the
launches the sorter makes under BWTC_HIP_MIXED=1, on the context's buffers.  k_p[], the longest stretch and the longest
PROPER stretch -- the largest k_p[s] over the s with s + 1 < n and T[s] != T[s + 1] -- are held to tests/periodmodel.py
and tests/mixedmodel.py by exact equality.  The blocks are tests/mixedcases.py's and tests/periodcases.py's;
tests/test_mixedmodel.py proves their premises without a GPU.

Without the feature the hook does not exist."""
import numpy as np
import pytest

import mixedcases as mc
import mixedmodel
import periodcases as pc
import periodmodel

pytestmark = pytest.mark.gpu

CAP = (1 << 20) + 4096
PERIODS = [p for p in pc.PERIODS if p > 1]


@pytest.fixture(scope="module")
def ctx():
    from bwtc_amd import hip
    c = hip.Context(0, CAP)
    yield c
    c.close()


def _same(ctx, T, p, what):
    want, longest = periodmodel.period_lengths_np(T, p)
    proper = mixedmodel.longest_proper_np(T, p, want)
    got, got_longest, got_proper = ctx.test_period_proper(T, p)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, p, T.size, "first difference at", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]), bad.size)
    assert (got_longest, got_proper) == (longest, proper), (what, p, T.size, got_longest, longest, got_proper, proper)
    return proper, longest


@pytest.mark.parametrize("p", PERIODS)
def test_the_named_blocks(ctx, p):
    """A block whose longest stretch is a run (proper < longest); runs of p - 1, p and p + 1 bytes beside a stretch; the
    one proper position on the last byte of a chunk, a wave's span, a tile and at n - 2; all-equal text (0); n <= p."""
    seen = {}
    for what, T in mc.proper_blocks(p):
        seen[what] = _same(ctx, T, p, what)
    proper, longest = seen["the longest stretch is a run"]
    assert 0 < proper < longest
    assert seen["all equal"][0] == 0


@pytest.mark.parametrize("p", PERIODS)
def test_every_size_and_the_seams(ctx, p):
    """The sizes and the seam blocks of the pass's own test: one stretch throughout, two-symbol noise, breaks around every
    seam -- the first maximum and the lengths must be what they are without the second."""
    for n in pc.lengths_of(p):
        _same(ctx, pc.stretch(p, n), p, "one stretch")
        _same(ctx, pc.two_symbols(n, p), p, "two symbols")
    S = pc.stretch(p, pc.SEAM_N)
    for delta in (-1, 0, 1):
        _same(ctx, pc.with_breaks(S, p, pc.seam_breaks(p, delta)), p, "seam %+d" % delta)
    _same(ctx, pc.with_breaks(S, p, pc.before_seam_breaks(p)), p, "p before the seams")
    # runs that end one byte before, on and behind every seam: the proper positions move across it
    for delta in (-1, 0, 1):
        T = np.repeat(np.arange(len(pc.SEAMS) + 1, dtype=np.uint8) + 3, np.diff([0] + sorted(q + delta for q in pc.SEAMS.values()) + [pc.SEAM_N + delta]))[:pc.SEAM_N]
        _same(ctx, T, p, "runs to the seams %+d" % delta)


def test_both_hooks_agree_and_refuse_alike(ctx):
    from bwtc_amd import hip
    big = pc.with_breaks(pc.stretch(257, (1 << 20) + 3), 257, [5000, 700000])
    big[300000:400000] = 0
    _same(ctx, big, 257, "large")
    k, longest = ctx.test_period_lengths(big, 257)
    k2, longest2, proper = ctx.test_period_proper(big, 257)
    assert (k == k2).all() and longest == longest2 and proper <= longest
    _same(ctx, np.array([5, 5, 6], np.uint8), 2, "tiny")
    _same(ctx, big, 1, "the general form of period 1")
    for T, p in ((big[:100], 0), (big[:100], 4097), (big[:0], 3), (np.zeros(CAP + (1 << 20), np.uint8), 3)):
        k_out = np.full(max(T.size, 4), 0xABCD1234, np.uint32)
        with pytest.raises(hip.BwtcHipError) as err:
            ctx.test_period_proper(T, p, k_out)
        assert err.value.code == -1 and (k_out == 0xABCD1234).all(), (T.size, p)
    _same(ctx, big, 257, "large again")
