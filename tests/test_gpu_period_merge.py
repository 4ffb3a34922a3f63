"""The merging stretch-length pass of BWTC_HIP_MULTI on the GPU (-m gpu), through the hook bwtc_hip_test_period_merge: the
launches the sorter makes when a closed-form step of a block with several periods is due, on the context's buffers.  The
merged words -- a look-up length in bits 0 ... 30, bit 31 for the members of the step -- are held to
tests/multimodel.py's merge_words() word for word, and the two maxima to tests/periodmodel.py and tests/mixedmodel.py, by
exact equality.  The blocks are tests/multicases.py's; tests/test_multimodel.py proves their premises without a GPU.

Without the feature the hook does not exist."""
import numpy as np
import pytest

import mixedmodel
import multicases as cases
import multimodel as mu
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


def _same(ctx, T, p, h, old, kp, maxima, what):
    """One pass (old None: fresh) against the model."""
    want = mu.merge_words(old, kp, h, fresh=old is None)
    got, longest, proper = ctx.test_period_merge(T, p, h, None if old is None else old.copy())
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, p, T.size, h, "first difference at", int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])), bad.size)
    assert (longest, proper) == maxima, (what, p, T.size, h, longest, proper, maxima)
    return want


@pytest.mark.parametrize("p", cases.MERGE_PERIODS)
def test_every_size_seam_old_word_and_depth(ctx, p):
    """n around a thread's 64 positions, a wave's 4096 and a tile's 16384, and several tiles; breaks one before, on and one
    after every such seam; the fresh and the merging form; old words all 0, equal to k_p, k_p + 1 and random with stale
    flags; the depth one below, at and one above a length that occurs."""
    took = kept = 0
    for n in cases.MERGE_SIZES:
        for delta in (-1, 0, 1):
            T = cases.merge_text(n, p, delta)
            kp, longest = periodmodel.period_lengths_np(T, p)
            maxima = (longest, mixedmodel.longest_proper_np(T, p, kp))
            for h in cases.merge_depths(kp):
                what = (n, delta)
                _same(ctx, T, p, h, None, kp, maxima, what + ("fresh",))
                for name, old in cases.merge_olds(kp, delta):
                    want = _same(ctx, T, p, h, old, kp, maxima, what + (name,))
                    took += int((want >> 31).sum())
                    kept += int(((want >> 31) == 0).sum())
    assert took > 0 and kept > 0, (took, kept)


def test_two_steps_in_a_row_and_another_period(ctx):
    """What a block does: a fresh step of one period, then the merging step of another over its words; the second step's
    members carry the flag, the first step's keep their lengths without it."""
    T = cases.stretches((9, 12), 1 << 15)
    k9, l9 = periodmodel.period_lengths_np(T, 9)
    k12, l12 = periodmodel.period_lengths_np(T, 12)
    first = _same(ctx, T, 9, 16, None, k9, (l9, mixedmodel.longest_proper_np(T, 9, k9)), "the first step")
    second = _same(ctx, T, 12, 16, first, k12, (l12, mixedmodel.longest_proper_np(T, 12, k12)), "the second step")
    in9 = np.flatnonzero((first >> 31) == 1)
    assert in9.size >= (1 << 15) - 16 and ((second[in9] >> 31) == 0).sum() >= in9.size - 64
    assert ((second & mu.LENGTH)[in9] >= k9[in9]).all() and ((second >> 31) == 1).sum() >= (1 << 15) - 16


def test_guarded_buffers_at_odd_alignments(ctx):
    """T at byte offsets 1 and 3 and the words at word offsets 1 and 3 of guarded host buffers: nothing outside is
    written."""
    for off in (1, 3):
        for n in (65, 4097, 2 * 16384 + 3):
            T0 = cases.merge_text(n, 9, 0)
            tbuf = np.full(n + 64, 0x5A, np.uint8)
            tbuf[off:off + n] = T0
            T = tbuf[off:off + n]
            kp, longest = periodmodel.period_lengths_np(T0, 9)
            old = cases.merge_olds(kp, off)[3][1]
            kbuf = np.full(n + 16, 0xABCD1234, np.uint32)
            kbuf[off:off + n] = old
            got, got_longest, _ = ctx.test_period_merge(T, 9, 12, kbuf[off:off + n])
            assert (got == mu.merge_words(old, kp, 12)).all() and got_longest == longest, (off, n)
            assert (kbuf[:off] == 0xABCD1234).all() and (kbuf[off + n:] == 0xABCD1234).all(), (off, n)
            assert (tbuf[:off] == 0x5A).all() and (tbuf[off + n:] == 0x5A).all() and (T == T0).all(), (off, n)


def test_one_context_large_tiny_refused_large(ctx):
    from bwtc_amd import hip
    big = pc.with_breaks(pc.stretch(257, (1 << 20) + 3), 257, [5000, 700000])
    kp, longest = periodmodel.period_lengths_np(big, 257)
    maxima = (longest, mixedmodel.longest_proper_np(big, 257, kp))
    old = cases.merge_olds(kp, 1)[3][1]
    _same(ctx, big, 257, 300000, old, kp, maxima, "large")
    tiny = np.array([5, 5, 6], np.uint8)
    k2, l2 = periodmodel.period_lengths_np(tiny, 2)
    _same(ctx, tiny, 2, 1, None, k2, (l2, mixedmodel.longest_proper_np(tiny, 2, k2)), "tiny")
    for T, p, h in ((big[:100], 0, 4), (big[:100], 4097, 4), (big[:0], 3, 4), (np.zeros(CAP + (1 << 20), np.uint8), 3, 4), (big[:100], 3, 0)):
        k = np.full(max(T.size, 4), 0xABCD1234, np.uint32)
        with pytest.raises(hip.BwtcHipError) as err:
            ctx.test_period_merge(T, p, h, k)
        assert err.value.code == -1 and (k == 0xABCD1234).all(), (T.size, p, h)
    _same(ctx, big, 257, 300000, old, kp, maxima, "large again")
    # the pass without the merge is what it was: the plain hook on the same context
    got, got_longest, got_proper = ctx.test_period_proper(big, 257)
    assert (got == kp).all() and (got_longest, got_proper) == maxima
