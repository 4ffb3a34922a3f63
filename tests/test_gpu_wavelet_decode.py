"""GPU tests of the 'B' / 'b' / 'u' device decode route (bwtc_hip_decode_block_W / _device): the host range-decodes
a record into a flattened forest, the device rebuilds the BWT bytes from it and inverts them.

Records come from the oracle's encoder and from the product's own; what is decoded is compared with the INPUT block,
never with anything the route under test made.  Every test proves from the statistics that the device kernels made
the bytes: launches, and runs / words / bit reads equal to what the host half and the host twin count for the
same record through a decoder handle of their own."""
import time

import numpy as np
import pytest

import wforest
from bwtc_amd import hip, synth

pytestmark = pytest.mark.gpu


def _route(ctx, counts, before):
    st = ctx.wavelet_decode_stats()
    assert st["route"] == 1 and st["launches"] > 0, st
    assert st["routed_device"] == before + 1, (st, before)
    for k in ("sections", "runs", "nodes", "words", "bit_reads"):
        assert st[k] == counts[k], (k, st, counts)
    return st


def _routed(ctx):
    return ctx.wavelet_decode_stats()["routed_device"]


def _structured(n, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 4000, max(2, n // 1500))
    return np.repeat(rng.integers(0, 6, lens.size).astype(np.uint8), lens)[:n]


def test_oracle_records_decode_to_the_input(hip_ctx, oracle):
    """Every letter, 1 / 8 / 256 starting points, one block and several through one handle."""
    for letter in "Bbu":
        for name, data in wforest.decoder_inputs() + [("C3_1M", synth.gen_text(1 << 20, 3))]:
            for sp, blocks in ((1, 1), (8, 3), (256, 1)):
                bs = data.size // blocks + (blocks > 1)
                coder, recs = wforest.records(oracle.oracle_compress_wavelet(letter, data, bs, sp))
                dec, counter = hip.WaveletDecoder(letter), hip.WaveletDecoder(letter)
                off = 0
                for n, rec in recs:
                    counts, _ = counter.counts(rec, n)
                    before = _routed(hip_ctx)
                    tail = np.concatenate([rec, np.full(19, 0xC3, np.uint8)])
                    back, used = hip_ctx.decode_block_W(dec, tail, cap=n, with_consumed=True)
                    assert used == rec.size and back.tobytes() == data[off:off + n].tobytes(), (letter, name, sp, off)
                    _route(hip_ctx, counts, before)
                    off += n
                assert off == data.size


_NAMES = ("C3", "random", "dna", "all_equal", "run_heavy")
_LETTERS, _STARTS = "Bbu", (1, 8, 256)
_made = {}


def _input(mib, name):
    """One input at a time (the 256 MiB ones are not kept side by side)."""
    if _made.get("key") != (mib, name):
        _made.clear()
        _made.update(key=(mib, name), data=dict(_inputs_one(mib << 20, name)))
    return _made["data"][name]


def _inputs_one(n, name):
    gen = {"C3": lambda: synth.gen_text(n, 3), "random": lambda: synth.gen_random_bytes(n, 1), "dna": lambda: synth.gen_dna(n, 2),
           "all_equal": lambda: np.full(n, 7, np.uint8), "run_heavy": lambda: _structured(n, 5)}
    return [(name, gen[name]())]


def _product_case(ctx, mib, name, letter, sp, oracle=None):
    n = mib << 20
    data = _input(mib, name)
    ctx.wavelet_start(letter)
    rec, _ = ctx.transform_and_encode_wavelet(data, sp)
    counter = hip.WaveletDecoder(letter)
    counts, used0 = counter.counts(rec, n)
    assert used0 == rec.size and counts["bytes"] == n
    if oracle is not None:                         # the rebuild surface on a real record, against the oracle's BWT bytes
        forest, lf = counter.forest()
        bwt, lf_ref, _ = oracle.oracle_bwt_block(data, sp)
        d = ctx.lib.bwtc_hip_malloc(ctx.handle, n + 64)
        try:
            before = _routed(ctx)
            assert ctx.wavelet_rebuild_device(forest, d + 3, n) == n
            got = np.empty(n, np.uint8)
            assert ctx.lib.bwtc_hip_memcpy_to_host(ctx.handle, got.ctypes.data, d + 3, n) == 0
            assert got.tobytes() == np.asarray(bwt, np.uint8).tobytes(), (name, letter, sp)
            assert list(lf) == list(lf_ref)
            _route(ctx, counts, before)
        finally:
            ctx.lib.bwtc_hip_free(ctx.handle, d)
    before = _routed(ctx)
    t0 = time.time()
    back = ctx.decode_block_W(hip.WaveletDecoder(letter), rec, cap=n)
    wall = time.time() - t0
    assert back.size == n and back.tobytes() == data.tobytes(), (name, letter, sp)
    st = _route(ctx, counts, before)
    print("%s %d MiB '%s' sp %d: decode_block_W %.2f s; range %.1f ms, rebuild %.2f ms (%d bit reads, %d words), inverse %.1f ms" %
          (name, mib, letter, sp, wall, st["ms_range_decode"], st["ms_rebuild"], st["bit_reads"], st["words"], st["ms_inverse"]))


@pytest.mark.parametrize("sp", _STARTS)
@pytest.mark.parametrize("letter", _LETTERS)
@pytest.mark.parametrize("name", _NAMES)
def test_product_records_1_mib(hip_ctx, oracle, name, letter, sp):
    """Every input x every letter x every number of starting points; the rebuild's BWT bytes against the oracle's."""
    _product_case(hip_ctx, 1, name, letter, sp, oracle)


def _rotated(mib):
    # above 1 MiB every input runs once per size, the letter and the starting points rotated so that each size sees
    # all three of both; the letter only picks the host's model set and the starting points only the LF powers the
    # inverse is given, and the full cross product of those two is run at 1 MiB above
    shift = {16: 0, 64: 1, 256: 2}[mib]
    return [(name, _LETTERS[(k + shift) % 3], _STARTS[(k + 2 * shift) % 3]) for k, name in enumerate(_NAMES)]


@pytest.mark.parametrize("mib,name,letter,sp", [(m,) + c for m in (16, 64) for c in _rotated(m)])
def test_product_records_16_and_64_mib(hip_ctx, oracle, mib, name, letter, sp):
    # the rebuild surface against orc_bwt_block up to 16 MiB: the oracle's transform is one CPU thread, seconds at
    # 16 MiB and minutes at 256; above that the rebuild's bytes are checked through the inverse, against the input
    _product_case(hip_ctx, mib, name, letter, sp, oracle if mib == 16 else None)


@pytest.fixture(scope="module")
def big_ctx():
    with hip.Context(0, 256 << 20) as ctx:
        yield ctx


@pytest.mark.parametrize("name,letter,sp", _rotated(256))
def test_product_records_256_mib(big_ctx, name, letter, sp):
    """The flagship block size (a context of its own: the shared one is sized for 64 MiB).  The range decoder is serial
    host code at some tens of nanoseconds per decision, twice per case (the counts and the decode), so the random and
    DNA cases of this size take tens of seconds each: DESIGN 8c has the figures."""
    _product_case(big_ctx, 256, name, letter, sp)


def test_begin_and_end_halves_with_two_slots(hip_ctx):
    """The split form: block k+1 range-decoded into the other slot before block k's device half runs."""
    blocks = [synth.gen_text(300_000 + 77 * k, 3 + k) for k in range(4)]
    hip_ctx.wavelet_start("B")
    recs = [hip_ctx.transform_and_encode_wavelet(b, 8)[0] for b in blocks]
    dec, counter = hip.WaveletDecoder("B"), hip.WaveletDecoder("B")
    counts = [counter.counts(r, b.size)[0] for r, b in zip(recs, blocks)]
    size, used = hip_ctx.decode_block_W_begin(dec, recs[0], blocks[0].size, 0)
    assert (size, used) == (blocks[0].size, recs[0].size)
    for k in range(4):
        if k + 1 < 4:
            size, used = hip_ctx.decode_block_W_begin(dec, recs[k + 1], blocks[k + 1].size, (k + 1) & 1)
            assert (size, used) == (blocks[k + 1].size, recs[k + 1].size)
        before = _routed(hip_ctx)
        back = hip_ctx.decode_block_W_end(k & 1, blocks[k].size)
        assert back.tobytes() == blocks[k].tobytes(), k
        _route(hip_ctx, counts[k], before)


def test_device_form_leaves_the_block_in_device_memory(hip_ctx):
    n = 3 << 20
    data = synth.gen_text(n, 3)
    hip_ctx.wavelet_start("B")
    rec, _ = hip_ctx.transform_and_encode_wavelet(data, 8)
    counts, _ = hip.WaveletDecoder("B").counts(rec, n)
    d = hip_ctx.lib.bwtc_hip_malloc(hip_ctx.handle, n + 64)
    try:
        for off in (0, 1, 7, 16):
            before = _routed(hip_ctx)
            size, used = hip_ctx.decode_block_W_device(hip.WaveletDecoder("B"), rec, d + off, n)
            assert size == n and used == rec.size
            back = np.empty(n, np.uint8)
            assert hip_ctx.lib.bwtc_hip_memcpy_to_host(hip_ctx.handle, back.ctypes.data, d + off, n) == 0
            assert back.tobytes() == data.tobytes(), off
            _route(hip_ctx, counts, before)
    finally:
        hip_ctx.lib.bwtc_hip_free(hip_ctx.handle, d)


def test_errors_leave_the_handle_usable(hip_ctx, oracle):
    data = synth.gen_text(200000, 3)
    _, recs = wforest.records(oracle.oracle_compress_wavelet("B", data, data.size, 8))
    rec = recs[0][1]
    dec = hip.WaveletDecoder("B")
    with pytest.raises(hip.BwtcHipError) as e:
        hip_ctx.decode_block_W(dec, rec[:rec.size // 2], cap=data.size)
    assert e.value.code == hip.E_PAST_RECORD
    with pytest.raises(hip.BwtcHipError) as e:
        hip_ctx.decode_block_W(dec, rec, cap=data.size - 1)
    assert e.value.code == hip.E_CAPACITY
    assert hip_ctx.decode_block_W(dec, rec, cap=data.size).tobytes() == data.tobytes()
