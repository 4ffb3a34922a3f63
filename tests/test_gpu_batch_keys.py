"""k_batch_load and k_batch_keys alone (-m gpu), through bwtc_hip_test_batch_keys: the reversed, terminated blocks, the
63-bit initial keys and the byte counts must equal tests/batchmodel.py exactly, at the load kernel's thread (16
positions), tile (4096 positions) and histogram (stride 256) seams, at strides that are just filled and just doubled,
at every source alignment and at the batch sizes where the block id gets another bit.

Without the feature every test fails: the entry point does not exist."""
import numpy as np
import pytest

import batchcases
import batchmodel

pytestmark = pytest.mark.gpu


def _check(ctx, blocks, first_offset=0, gap=0):
    """the blocks at first_offset, `gap` bytes of 0xEE between them (and around them)"""
    blocks = [np.ascontiguousarray(b, np.uint8) for b in blocks]
    offsets, at = [], first_offset
    for b in blocks:
        offsets.append(at)
        at += b.size + gap
    data = np.full(at + 16, 0xEE, np.uint8)
    for b, off in zip(blocks, offsets):
        data[off:off + b.size] = b
    T, keys, counts = ctx.test_batch_keys(data, offsets, [b.size for b in blocks])
    wT, wkeys, wcounts = batchmodel.keys_and_text(blocks)
    assert T.size == wT.size and (T == wT).all(), np.flatnonzero(T != wT)[:8]
    assert (keys == wkeys).all(), np.flatnonzero(keys != wkeys)[:8]
    assert (counts[:len(blocks)] == wcounts).all()


def _blocks(sizes, seed=1, sigma=256):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, sigma, s, dtype=np.uint8) for s in sizes]


SMALL_SIZES = [1, 2, 5, 6, 7, 15, 16, 17]


@pytest.mark.parametrize("size", SMALL_SIZES)
def test_one_small_block(hip_ctx, size):
    _check(hip_ctx, _blocks([size], size))


def test_small_blocks_together(hip_ctx):
    _check(hip_ctx, _blocks(SMALL_SIZES + SMALL_SIZES[::-1], 2, 3))


@pytest.mark.parametrize("seam", [batchcases.LOAD_PER_THREAD, 2 * batchcases.LOAD_PER_THREAD, batchcases.LDS_HIST_FROM,
                                  batchcases.LOAD_TILE, 2 * batchcases.LOAD_TILE])
def test_thread_tile_and_histogram_seams(hip_ctx, seam):
    # sizes around the seam, and n_b (size + 1) around it
    sizes = [seam - 2, seam - 1, seam, seam + 1, seam + 2]
    for size in sizes:
        _check(hip_ctx, _blocks([size], seam + size, 5))
    _check(hip_ctx, _blocks(sizes, seam, 2))


@pytest.mark.parametrize("k", range(1, 15))
def test_stride_filled_and_doubled(hip_ctx, k):
    full, over = (1 << k) - 1, 1 << k
    assert batchmodel.stride_log2([full]) == k and batchmodel.stride_log2([over]) == k + 1
    _check(hip_ctx, _blocks([full, full, full], k, 4))                 # n_b = S: no padding anywhere
    _check(hip_ctx, _blocks([over, 1, over], k, 4))                    # n_b = S / 2 + 1


@pytest.mark.parametrize("offset", [0, 1, 7, 15, 16, 17, 31])
def test_source_offsets(hip_ctx, offset):
    for gap in (0, 1, 16):
        _check(hip_ctx, _blocks([100, 4096, 33, 5000], offset + gap), offset, gap)


@pytest.mark.parametrize("count", [1, 2, 64, 65, 256, 257, 4096])
def test_block_counts(hip_ctx, count):
    rng = np.random.default_rng(count)
    sizes = rng.integers(1, 41, count).tolist()
    assert batchmodel.stride_log2(sizes) <= 6
    _check(hip_ctx, _blocks(sizes, count, 3))
    if count in (65, 4096):                                            # stride 256 and more: the LDS histograms, 16 blocks a workgroup
        _check(hip_ctx, _blocks([int(s) + 215 for s in sizes], count, 2))


def test_zeros(hip_ctx):
    rng = np.random.default_rng(9)
    lead = [np.concatenate([np.zeros(z, np.uint8), rng.integers(0, 3, r, dtype=np.uint8)])
            for z, r in ((1, 1), (5, 1), (6, 3), (7, 20), (300, 5), (5000, 100))]
    zeros = [np.zeros(s, np.uint8) for s in (1, 2, 5, 6, 7, 16, 17, 255, 256, 4096, 4097)]
    _check(hip_ctx, lead)
    _check(hip_ctx, zeros)
    _check(hip_ctx, [b[::-1] for b in lead] + zeros + lead)
