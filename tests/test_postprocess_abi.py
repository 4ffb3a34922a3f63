"""CPU tests of the device postprocessor's boundary (`--prepr` blocks, Postprocessor::uncompress,
preprocessors/Postprocessor.cpp:62-133): the entry points are declared and bound, their argument checks need no
device, and the host twin of the kernels' passes -- expansion table, run starts carried over tiles, per-tile counts,
offsets, the write pass's search from the output's side -- agrees with the host function (bwtc_hip_postprocess,
existing code) on precompressed blocks and on data that no precompressor wrote."""
import os
import re

import numpy as np
import pytest

from test_host_logic import _prepr_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bwtc_hip_postprocess_device", "bwtc_hip_postprocess_block", "bwtc_hip_decode_block_H_device",
       "bwtc_hip_postprocess_stats_get"]
TILES = (16, 64, 4096)


def special_grammar():
    """The "ppppp" grammar of the first _prepr_inputs() case with at least two special symbols, and that case's
    precompressed block."""
    from bwtc_amd import hip
    for name, data in _prepr_inputs():
        g = hip.Grammar()
        pre = g.host_precompress("ppppp", data)
        if g.special_symbols >= 2:
            return g, pre, data
    raise AssertionError("no _prepr_inputs() case has two special symbols after ppppp")


def arbitrary_cases(g):
    """Data that no precompressor wrote, under a real grammar with special symbols."""
    specials = np.array([c for c in range(256) if g.is_special(c)], np.uint8)
    plain = np.array([c for c in range(256) if not g.is_special(c)], np.uint8)
    assert specials.size >= 2
    rng = np.random.default_rng(17)
    out = []
    # (a) runs of one special byte of every length 1..70 between bytes that are not special
    parts = []
    for k in range(1, 71):
        parts += [np.full(k, specials[k % specials.size], np.uint8), plain[rng.integers(0, plain.size, 1 + k % 3)]]
    out.append(("runs_1_70", np.concatenate(parts)))
    # (b) runs of mixed special bytes that span tile seams at both parities
    for k in (4095, 4096, 4097, 3 * 4096 + 1, 100001):
        run = specials[rng.integers(0, specials.size, k)]
        out.append(("mixed_run_%d" % k, np.concatenate([plain[:5], run, plain[5:12], run[:k // 2], plain[:3]])))
        out.append(("mixed_run_%d_first" % k, np.concatenate([run, plain[:2]])))
    # (c) the last byte is special: a single-byte token
    # (long enough for the expansion to hold any single rule's: the host function's guard refuses a smaller max_size)
    out.append(("last_special", np.concatenate([np.tile(plain, 20), specials[:1]])))
    out.append(("last_special_after_run", np.concatenate([np.tile(plain, 20), specials[[0, 1, 0]]])))
    # (d) uniform random bytes
    out.append(("random_1MiB", rng.integers(0, 256, 1 << 20).astype(np.uint8)))
    return out


def _header():
    text = open(os.path.join(ROOT, "include", "bwtc_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_new_entry_points_are_declared_and_bound():
    from bwtc_amd import hip
    lib = hip.load()
    text = _header()
    for name in NEW + ["bwtc_hip_host_postprocess_tiles"]:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert "bwtc_hip_postprocess_stats" in text
    for method in ("postprocess", "postprocess_device", "decode_block_H_device", "postprocess_stats"):
        assert callable(getattr(hip.Context, method)), method
    fields = [f for f, _ in hip.PostprocessStats._fields_]
    for f in ("route", "tokens", "pair_tokens", "in_bytes", "out_bytes", "pool_bytes", "launches", "workspace_bytes", "ms_device"):
        assert f in fields and re.search(r"\b%s;" % f, text), f


def test_null_arguments_return_minus_one():
    import ctypes
    from bwtc_amd import hip
    lib = hip.load()
    g = hip.Grammar()
    buf = np.zeros(16, np.uint8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    n = ctypes.c_uint64(0)
    size = ctypes.c_uint32(0)
    fake_ctx = ctypes.c_void_p(1)                                   # never dereferenced: a later argument is refused first
    for f in (lib.bwtc_hip_postprocess_device, lib.bwtc_hip_postprocess_block):
        assert f(None, g.h, p, 4, p, 16, ctypes.byref(n)) == -1      # null context
        assert f(fake_ctx, None, p, 4, p, 16, ctypes.byref(n)) == -1    # null grammar
        assert f(fake_ctx, g.h, None, 4, p, 16, ctypes.byref(n)) == -1  # null data
        assert f(fake_ctx, g.h, p, 4, None, 16, ctypes.byref(n)) == -1  # null output
        assert f(fake_ctx, g.h, p, 4, p, 16, None) == -1                # null size
    assert lib.bwtc_hip_decode_block_H_device(None, p, 16, p, 16, ctypes.byref(size), ctypes.byref(n)) == -1
    assert lib.bwtc_hip_decode_block_H_device(fake_ctx, None, 16, p, 16, ctypes.byref(size), ctypes.byref(n)) == -1
    assert lib.bwtc_hip_decode_block_H_device(fake_ctx, p, 16, None, 16, ctypes.byref(size), ctypes.byref(n)) == -1
    assert lib.bwtc_hip_decode_block_H_device(fake_ctx, p, 16, p, 16, None, ctypes.byref(n)) == -1
    assert lib.bwtc_hip_decode_block_H_device(fake_ctx, p, 16, p, 16, ctypes.byref(size), None) == -1
    assert lib.bwtc_hip_postprocess_stats_get(None, ctypes.byref(hip.PostprocessStats())) == -1
    assert lib.bwtc_hip_postprocess_stats_get(fake_ctx, None) == -1
    assert lib.bwtc_hip_host_postprocess_tiles(None, p, 4, p, 16, ctypes.byref(n), 16) == -1
    assert lib.bwtc_hip_host_postprocess_tiles(g.h, None, 4, p, 16, ctypes.byref(n), 16) == -1
    assert lib.bwtc_hip_host_postprocess_tiles(g.h, p, 4, None, 16, ctypes.byref(n), 16) == -1
    assert lib.bwtc_hip_host_postprocess_tiles(g.h, p, 4, p, 16, None, 16) == -1
    assert lib.bwtc_hip_host_postprocess_tiles(g.h, p, 4, p, 16, ctypes.byref(n), 0) == -1


@pytest.mark.parametrize("name,data", _prepr_inputs(), ids=[n for n, _ in _prepr_inputs()])
def test_tile_twin_expands_precompressed_blocks_like_the_host_function(name, data):
    from bwtc_amd import hip
    for opts in ("p", "pp", "ppppp"):
        g = hip.Grammar()
        pre = g.host_precompress(opts, data)
        want = g.postprocess(pre, data.size + 8)
        assert want.tobytes() == data.tobytes()
        for tile in TILES:
            got = g.host_postprocess_tiles(pre, data.size, tile)     # the exact size is enough room
            assert got.size == want.size and (got == want).all(), (name, opts, tile)


def test_tile_twin_expands_arbitrary_data_like_the_host_function():
    g, _, _ = special_grammar()
    for name, data in arbitrary_cases(g):
        want = g.postprocess(data, 64 * data.size + 64)
        for tile in TILES:
            got = g.host_postprocess_tiles(data, want.size, tile)
            assert got.size == want.size and (got == want).all(), (name, tile)


def test_tile_twin_refuses_what_does_not_fit_and_writes_nothing():
    import ctypes
    from bwtc_amd import hip
    lib = hip.load()
    g, pre, data = special_grammar()
    n = ctypes.c_uint64(0)
    for tile in TILES:
        out = np.full(data.size, 0xA5, np.uint8)
        rc = lib.bwtc_hip_host_postprocess_tiles(g.h, pre.ctypes.data_as(ctypes.c_void_p), pre.size, out.ctypes.data_as(ctypes.c_void_p),
                                                 data.size - 1, ctypes.byref(n), tile)
        assert rc == -1 and (out == 0xA5).all()
        with pytest.raises(hip.BwtcHipError):
            g.postprocess(pre, data.size - 1)


def test_tile_twin_copies_under_a_grammar_without_rules():
    from bwtc_amd import hip
    g = hip.Grammar()
    for n in (0, 1, 2, 3, 100):
        data = np.arange(n, dtype=np.uint8)
        assert g.host_postprocess_tiles(data, n, 16).tobytes() == data.tobytes()
