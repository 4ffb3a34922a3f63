"""The batched block transform on the GPU (-m gpu): bytes, LF powers and counts of every block against
oracle.oracle_bwt_block, the rounds and the entries left after each against tests/batchmodel.py, on the named batches
of tests/batchcases.py (whose premises tests/test_batchmodel.py proves) -- and the property the feature exists for:
the host waits of a call do not grow with the number of blocks.

Without the feature every test fails: the entry points do not exist."""
import ctypes

import numpy as np
import pytest

import batchcases
import batchmodel

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    assert len(got) == len(want), what
    for b, (g, w) in enumerate(zip(got, want)):
        for part, x, y in zip(("bytes", "lf", "freqs"), g, w):
            assert x.shape == y.shape and (x == y).all(), (what, b, part)


def _stats_equal_model(ctx, res, k):
    st = ctx.batch_stats()
    assert st["blocks"] == k and st["stride_log2"] == res["k"] and st["suffixes"] == res["suffixes"]
    assert st["rounds"] == res["rounds"], (st["rounds"], res["rounds"])
    assert st["active"] == res["active"][:32]
    return st


@pytest.mark.parametrize("name", sorted(batchcases.CASES))
def test_named_batches(hip_ctx, oracle, name):
    blocks, sp = batchcases.case(name)
    got = hip_ctx.bwt_blocks(blocks, sp)
    _same(got, batchcases.oracle(name), name)
    st = _stats_equal_model(hip_ctx, batchcases.model(name), len(blocks))
    assert st["host_waits"] <= st["rounds"] + 4


def test_one_block_is_the_single_transform(hip_ctx, oracle):
    rng = np.random.default_rng(21)
    for size, sigma in ((1, 2), (2, 2), (300, 2), (5000, 4), (70000, 256)):
        block = rng.integers(0, sigma, size, dtype=np.uint8)
        got = hip_ctx.bwt_blocks([block], 8)
        _same(got, [oracle.oracle_bwt_block(block, 8)], size)
        _same(got, [hip_ctx.bwt_block(block, 8)], size)
        _stats_equal_model(hip_ctx, batchmodel.transform([block], 8), 1)


def test_hundred_mixed_batches_on_one_context(hip_ctx, oracle):
    rng = np.random.default_rng(22)
    for i in range(100):
        blocks, sp = batchcases.random_batch(rng)
        got = hip_ctx.bwt_blocks(blocks, sp)
        _same(got, [oracle.oracle_bwt_block(b, sp) for b in blocks], i)
        _stats_equal_model(hip_ctx, batchmodel.transform(blocks, sp), len(blocks))


def _device_layout(blocks, guard):
    offsets, at = [], guard
    for b in blocks:
        offsets.append(at)
        at += b.size + guard
    buf = np.full(at, 0xC7, np.uint8)
    for b, off in zip(blocks, offsets):
        buf[off:off + b.size] = b
    return buf, offsets


@pytest.mark.parametrize("guard", [0, 1, 16])
@pytest.mark.parametrize("in_place", [True, False])
def test_device_form_and_guard_bytes(hip_ctx, oracle, guard, in_place):
    rng = np.random.default_rng(23 + guard)
    blocks = [rng.integers(0, 4, s, dtype=np.uint8) for s in (1, 17, 4096, 300, 5, 9000, 2)]
    buf, offsets = _device_layout(blocks, guard)
    sizes = [b.size for b in blocks]
    d_in = hip_ctx.dmalloc(buf.size)
    d_out = d_in if in_place else hip_ctx.dmalloc(buf.size)
    try:
        hip_ctx.to_device(d_in, buf)
        if not in_place:
            hip_ctx.to_device(d_out, np.full(buf.size, 0x5A, np.uint8))
        lf, freqs, n_lfs = hip_ctx.bwt_blocks_device(d_in, d_out, offsets, sizes, 8)
        out = hip_ctx.to_host(d_out, buf.size)
        if not in_place:
            assert (hip_ctx.to_host(d_in, buf.size) == buf).all()      # the source is read only
    finally:
        hip_ctx.dfree(d_in)
        if not in_place:
            hip_ctx.dfree(d_out)
    want = [oracle.oracle_bwt_block(b, 8) for b in blocks]
    got = [(out[off:off + s], lf[i, :n_lfs[i]], freqs[i]) for i, (off, s) in enumerate(zip(offsets, sizes))]
    _same(got, want, "device")
    inside = np.zeros(buf.size, bool)
    for off, s in zip(offsets, sizes):
        inside[off:off + s] = True
    assert (out[~inside] == (0xC7 if in_place else 0x5A)).all()        # no byte outside a block is written
    assert (lf[np.arange(256)[None, :] >= np.array(n_lfs)[:, None]] == 0).all()


def test_refusals_leave_the_buffer_alone(hip_ctx):
    from bwtc_amd import hip
    rng = np.random.default_rng(24)
    buf = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    keep = buf.copy()
    lf = np.full((8, 256), 7, np.uint32)
    freqs = np.full((8, 256), 7, np.uint32)

    def call(items, k=None):
        arr = (hip.BatchItem * max(len(items), 1))()
        for i, (off, size, n_lf) in enumerate(items):
            arr[i].offset, arr[i].size, arr[i].n_lf = off, size, n_lf
        return hip_ctx.lib.bwtc_hip_bwt_blocks(hip_ctx.handle, buf.ctypes.data_as(ctypes.c_void_p), ctypes.cast(arr, ctypes.c_void_p),
                                               len(items) if k is None else k, lf.ctypes.data_as(ctypes.c_void_p),
                                               freqs.ctypes.data_as(ctypes.c_void_p))

    ok = [(0, 100, 1), (100, 100, 1)]                                   # blocks may touch
    refused = {
        "k == 0": (ok, 0),
        "size == 0": ([(0, 100, 1), (200, 0, 1)], None),
        "n_lf == 0": ([(0, 100, 0)], None),
        "n_lf > 256": ([(0, 300, 257)], None),
        "overlap": ([(0, 100, 1), (99, 100, 1)], None),
        "overlap, out of order": ([(500, 100, 1), (0, 100, 1), (450, 51, 1)], None),
        "same block twice": ([(0, 100, 1), (0, 100, 1)], None),
    }
    for what, (items, k) in refused.items():
        assert call(items, k) == -1, what
        assert (buf == keep).all() and (lf == 7).all() and (freqs == 7).all(), what
    many = [(i, 1, 1) for i in range(4097)]
    big_lf = np.zeros((4097, 256), np.uint32)
    arr = (hip.BatchItem * 4097)()
    for i, (off, size, n_lf) in enumerate(many):
        arr[i].offset, arr[i].size, arr[i].n_lf = off, size, n_lf
    assert hip_ctx.lib.bwtc_hip_bwt_blocks(hip_ctx.handle, buf.ctypes.data_as(ctypes.c_void_p), ctypes.cast(arr, ctypes.c_void_p), 4097,
                                           big_lf.ctypes.data_as(ctypes.c_void_p), None) == -1
    assert (buf == keep).all()
    # k * S above max_block_size + 1: a context of 4095 bytes holds one stride of 4096 and not two
    with hip.Context(0, 4095) as small:
        one = small.bwt_blocks([keep[:4095]], 1)
        assert one[0][0].size == 4095
        with pytest.raises(hip.BwtcHipError) as err:
            small.bwt_blocks([keep[:4095], keep[:1]], 1)
        assert err.value.args[0].endswith("-1")
        with pytest.raises(hip.BwtcHipError):
            small.bwt_blocks([keep[:4096]], 1)                          # the stride doubles to 8192
    assert call(ok) == 0 and not (buf == keep).all()                   # and what is not refused runs


def test_batch_single_batch_on_one_context(oracle):
    from bwtc_amd import hip, synth
    text = np.ascontiguousarray(synth.gen_text(300000, 4)[:300000])
    batch = [text[i * 3000:(i + 1) * 3000] for i in range(40)]
    fields = [f for f, _ in hip.Stats._fields_ if not f.startswith("ms")]
    with hip.Context(0, 1 << 20) as fresh:
        want = fresh.bwt_block(text, 8)
        want_stats = fresh.stats()
    with hip.Context(0, 1 << 20) as ctx:
        first = ctx.bwt_blocks(batch, 8)
        got = ctx.bwt_block(text, 8)
        got_stats = ctx.stats()
        second = ctx.bwt_blocks(batch, 8)
    _same([got], [want], "single block between two batches")
    _same([got], [oracle.oracle_bwt_block(text, 8)], "single block")
    for f in fields:
        assert getattr(got_stats, f) == getattr(want_stats, f), f
    _same(first, second, "batch before and after")
    _same(first, [oracle.oracle_bwt_block(b, 8) for b in batch], "batch")


def test_host_waits_do_not_grow_with_the_batch(hip_ctx):
    rng = np.random.default_rng(25)
    block = rng.integers(0, 3, 250, dtype=np.uint8)
    waits = {}
    for k in (1, 4096):
        hip_ctx.bwt_blocks([block] * k, 8)
        st = hip_ctx.batch_stats()
        assert st["blocks"] == k
        assert st["host_waits"] <= st["rounds"] + 4, st
        waits[k] = (st["host_waits"], st["rounds"])
    assert waits[1] == waits[4096]                                     # the same block 4096 times: the same rounds, the same waits
