"""GPU tests of the wavelet rebuild kernels at their limits (bwtc_hip_wavelet_rebuild / _device): the hand-built
forests of tests/wforest.py -- written the way the encoder fills the nodes, so the expected bytes are the runs
themselves -- with the output at all 16 offsets from alignment, and malformed forests, which the kernels must refuse
with their own code and without a byte written past the capacity.  Every loop of the kernels is bounded, so a
malformed forest is an ordinary input here."""
import numpy as np
import pytest

import wforest
from bwtc_amd import hip

pytestmark = pytest.mark.gpu
GUARD = 64


def _device_rebuild(ctx, forest, cap, offset=0):
    """Rebuild into guarded device memory at `offset` from a 256-byte boundary: (bytes, error code, guard intact)."""
    L, h = ctx.lib, ctx.handle
    room = offset + cap + GUARD
    d = L.bwtc_hip_malloc(h, room + 256)
    assert d
    try:
        base = (d + 255) // 256 * 256
        fill = np.full(room, 0xA5, np.uint8)
        assert L.bwtc_hip_memcpy_to_device(h, base, fill.ctypes.data, room) == 0
        code, size = 0, 0
        try:
            size = ctx.wavelet_rebuild_device(forest, base + offset, cap)
        except hip.BwtcHipError as e:
            code = e.code
        back = np.empty(room, np.uint8)
        assert L.bwtc_hip_memcpy_to_host(h, back.ctypes.data, base, room) == 0
        intact = (back[:offset] == 0xA5).all() and (back[offset + cap:] == 0xA5).all()
        return back[offset:offset + size].copy(), code, bool(intact)
    finally:
        L.bwtc_hip_free(h, d)


@pytest.mark.parametrize("name", sorted(wforest.cases()))
def test_hand_built_forests_at_every_alignment(hip_ctx, name):
    sections, gap = wforest.cases()[name]
    forest, runs, reads = wforest.pack(sections, gap)
    want = wforest.expand(runs)
    for offset in range(16):
        before = hip_ctx.wavelet_decode_stats()["routed_device"]
        got, code, intact = _device_rebuild(hip_ctx, forest, want.size, offset)
        assert code == 0 and intact, (name, offset, code)
        assert got.size == want.size and got.tobytes() == want.tobytes(), (name, offset)
        st = hip_ctx.wavelet_decode_stats()
        assert st["route"] == 1 and st["launches"] > 0 and st["routed_device"] == before + 1, st
        assert st["runs"] == len(runs) and st["words"] == forest.words.size and st["bit_reads"] == reads, (name, st)
    assert hip_ctx.wavelet_rebuild(forest).tobytes() == want.tobytes()      # host to host


def test_host_twin_agrees_on_counts(hip_ctx):
    for name, (sections, gap) in wforest.cases().items():
        forest, runs, reads = wforest.pack(sections, gap)
        _, twin_reads = hip.host_wavelet_rebuild(forest)
        hip_ctx.wavelet_rebuild(forest)
        assert hip_ctx.wavelet_decode_stats()["bit_reads"] == twin_reads == reads, name


def test_line_count_scan_goes_from_one_launch_to_three(hip_ctx):
    """4096 lines of 7 words are one tile of the scan over the line counts; one word more is a 4097th line."""
    launches = []
    for w in wforest.WORD_COUNTS:
        sections, gap = wforest.cases()["words_%d" % w]
        forest, runs, reads = wforest.pack(sections, gap)
        assert forest.words.size == w
        assert hip_ctx.wavelet_rebuild(forest).tobytes() == wforest.expand(runs).tobytes(), w
        st = hip_ctx.wavelet_decode_stats()
        assert st["words"] == w and st["bit_reads"] == reads, st
        launches.append(st["launches"])
    assert launches[0] == launches[1] and launches[2] == launches[1] + 2 and launches[3] == launches[2], launches


def test_run_of_2_pow_31_minus_1(hip_ctx):
    n = (1 << 31) - 1
    forest, runs, reads = wforest.pack([wforest.section([(200, n)], W=15)])
    L, h = hip_ctx.lib, hip_ctx.handle
    d = L.bwtc_hip_malloc(h, n + 1 + GUARD)
    assert d
    try:
        fill = np.full(GUARD, 0xA5, np.uint8)
        assert L.bwtc_hip_memcpy_to_device(h, d + n, fill.ctypes.data, GUARD) == 0
        assert hip_ctx.wavelet_rebuild_device(forest, d, n) == n
        st = hip_ctx.wavelet_decode_stats()
        assert st["route"] == 1 and st["runs"] == 1 and st["bit_reads"] == reads, st
        back = np.empty(1 << 28, np.uint8)
        for a in range(0, n + GUARD, 1 << 28):
            k = min(1 << 28, n + GUARD - a)
            assert L.bwtc_hip_memcpy_to_host(h, back.ctypes.data, d + a, k) == 0
            body = max(0, min(k, n - a))
            assert (back[:body] == 200).all() and (back[body:k] == 0xA5).all(), a
    finally:
        L.bwtc_hip_free(h, d)


@pytest.mark.parametrize("name", sorted(wforest.corrupt_cases()))
def test_corrupt_forests_are_refused_with_their_code(hip_ctx, name):
    forest, cap, code = wforest.corrupt_cases()[name]
    for offset in (0, 5):
        before = hip_ctx.wavelet_decode_stats()["routed_device"]
        _, got, intact = _device_rebuild(hip_ctx, forest, cap, offset)
        assert got == code, (name, got, code)
        assert intact, name
        st = hip_ctx.wavelet_decode_stats()
        assert st["route"] == 0 and st["routed_device"] == before, st
    # and a good forest still rebuilds afterwards
    good, runs, _ = wforest.pack(wforest.cases()["five_sections"][0], 1)
    assert hip_ctx.wavelet_rebuild(good).tobytes() == wforest.expand(runs).tobytes()
