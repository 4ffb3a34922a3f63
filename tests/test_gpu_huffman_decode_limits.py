"""The GPU 'H' decoder (bwtc_hip_huffman_decode / _device) at its code, tile, window and size limits.

Records come from the oracle's encoder (the coders' limit blocks) or from the test-side writer
(tests/hrecord.py: any prefix-free code up to 64 bits, any section split, damage of one named kind),
whose expected bytes are np.repeat(run symbols, run lengths).  Every decode compares all bytes, the
LF powers and the bytes consumed, and checks that the device route made them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import blockgen
import hrecord
from bwtc_amd import hip, synth
from test_coder_limits import frame
from test_gpu_huffman_decode import _decode_guarded

pytestmark = pytest.mark.gpu
GUARD = 4096
FILL = 0xE7


def _stats(ctx):
    st = ctx.huffman_decode_stats()
    assert st["route"] == 1, st
    return st


def _decode(ctx, rec, facts, buf=None):
    """huffman_decode of `rec` (or of `buf`, the record and what follows it) against the facts."""
    total = facts["total"]
    got, lf, used = ctx.huffman_decode(rec if buf is None else buf, cap=max(total, 1))
    assert used == rec.size and used == facts["bytes"]
    assert lf.tolist() == facts["lf"]
    assert got.size == total and (got == hrecord.expected(facts)).all()
    st = _stats(ctx)
    assert st["runs"] == sum(s["n_runs"] for s in facts["sections"])
    assert st["sections"] == sum(s["S"] > 0 for s in facts["sections"])
    return st


def _device_decode(ctx, rec, cap, rec_off, out_off):
    """huffman_decode_device with the record at d_rec + rec_off and the output at d_out + out_off, a
    guard of GUARD bytes before and after the output: returns (bytes, LF powers, consumed)."""
    d_rec = ctx.dmalloc(rec_off + rec.size)
    n = GUARD + out_off + cap + GUARD
    d_out = ctx.dmalloc(n)
    try:
        ctx.to_device(d_rec + rec_off, rec)
        ctx.to_device(d_out, np.full(n, FILL, np.uint8))
        size, lf, used = ctx.huffman_decode_device(d_rec + rec_off, rec.size, d_out + GUARD + out_off, cap)
        back = np.empty(n, np.uint8)
        assert ctx.lib.bwtc_hip_memcpy_to_host(ctx.handle, back.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_out),
                                               n) == 0
        a = GUARD + out_off
        assert (back[:a] == FILL).all(), "guard before the output written"
        assert (back[a + size:] == FILL).all(), "guard after the output written"
        return back[a:a + size], lf, used
    finally:
        ctx.dfree(d_rec)
        ctx.dfree(d_out)


# record at device offsets 1, 3, 7; output at offset 0 (the expansion's direct path) and 1, 8, 15 (copy)
PLACEMENTS = [(1, 0), (3, 1), (7, 8), (1, 15), (3, 0)]


# ---- 1. the coders' limit blocks ---------------------------------------------------------------------

@pytest.mark.parametrize("name", blockgen.LIMIT_CASE_NAMES)
def test_limit_blocks(name, hip_ctx, oracle):
    [(_, block, _)] = list(blockgen.limit_blocks(names=(name,)))
    freqs = np.bincount(block, minlength=256).astype(np.uint32)
    rec = oracle.oracle_huffman_encode_block(block, np.zeros(1, np.uint32), freqs)
    sections = oracle.oracle_sections(freqs)
    m = blockgen.limit_measures(block, oracle)
    got, lf, used = hip_ctx.huffman_decode(rec)
    assert used == rec.size and lf.tolist() == [0]
    assert got.size == block.size and (got == block).all(), name
    st = _stats(hip_ctx)
    assert st["runs"] == sum(s.size for s, _ in blockgen.section_runs(block, sections)), (name, st)
    assert st["sections"] == np.count_nonzero(sections), (name, st)
    assert st["max_code_len"] == m["max_code_len_H"], (name, st, m)
    if name == "fib_depth":
        assert st["max_code_len"] >= 34
    for rec_off, out_off in PLACEMENTS:
        back, lf, used = _device_decode(hip_ctx, rec, block.size, rec_off, out_off)
        assert used == rec.size and lf.tolist() == [0]
        assert back.size == block.size and (back == block).all(), (name, rec_off, out_off)
        _stats(hip_ctx)


# ---- 2. code shapes ------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_len", hrecord.CODE_SHAPE_MAX_LENS)
def test_code_shapes(max_len, hip_ctx):
    rec, facts = hrecord.code_shape_case(max_len)
    st = _decode(hip_ctx, rec, facts)
    assert st["max_code_len"] == max_len, st
    back, lf, used = _device_decode(hip_ctx, rec, facts["total"], 3, 8)
    assert used == rec.size and (back == hrecord.expected(facts)).all()


def test_incomplete_prefix_free_code(hip_ctx):
    rec, facts = hrecord.incomplete_case()
    st = _decode(hip_ctx, rec, facts)
    assert st["max_code_len"] == 2


# ---- 3. the soft Huffman window's retry ----------------------------------------------------------------

def test_soft_window_retry(hip_ctx):
    rec, facts = hrecord.retry_case()
    st = _decode(hip_ctx, rec, facts)
    assert st["retries"] == 1 and st["max_code_len"] == 64, st
    assert st["host_syncs"] == st["sections"] + 1, st
    print("retry: %s" % {k: st[k] for k in ("retries", "max_code_len", "tiles", "host_syncs")})


# ---- 4. the map tree's levels --------------------------------------------------------------------------

@pytest.mark.parametrize("name,n_runs,tiles", hrecord.huffman_tile_runs())
def test_huffman_stream_tiles(name, n_runs, tiles, hip_ctx):
    rec, facts = hrecord.huffman_tiles_case(n_runs)
    assert facts["sections"][0]["h_tiles"] == tiles
    st = _decode(hip_ctx, rec, facts)
    assert st["tiles"] >= tiles and st["retries"] == 0, st


@pytest.mark.parametrize("name,n_runs,width,tiles", hrecord.gamma_tile_runs())
def test_gamma_stream_tiles(name, n_runs, width, tiles, hip_ctx):
    rec, facts = hrecord.gamma_tiles_case(n_runs, width)
    sec = facts["sections"][0]
    assert sec["g_tiles"] == tiles
    st = _decode(hip_ctx, rec, facts)
    assert st["tiles"] >= sec["h_tiles"] + tiles, st
    if tiles == 262145:
        print("%s: %d tiles" % (name, st["tiles"]))


# ---- 5. sections ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c[0] for c in hrecord.sections_cases()])
def test_sections(name, hip_ctx):
    [(_, (rec, facts))] = [c for c in hrecord.sections_cases() if c[0] == name]
    _decode(hip_ctx, rec, facts)
    back, lf, used = _device_decode(hip_ctx, rec, facts["total"], 7, 15)
    assert used == rec.size and lf.tolist() == facts["lf"] and (back == hrecord.expected(facts)).all()


def test_tail_of_valid_codes(hip_ctx):
    """The record is followed by bytes that parse as codes (the record again, then its streams): only
    the record the length field announces is decoded."""
    rec, facts = hrecord.code_shape_case(13)
    at = facts["sections"][0]["at"]
    buf = np.concatenate([rec, rec, rec[at["huffman"]:], rec[at["gamma"]:]])
    _decode(hip_ctx, rec, facts, buf)


# ---- 6. the 32-bit ceiling -----------------------------------------------------------------------------

def test_32_bit_ceiling():
    """A block of exactly 0xFFFFFFF0 bytes with a run of 2^31 + 1 bytes (a 63-bit gamma code) decodes on
    the device; one byte more is E_CAPACITY.  A context of its own: the decoder's workspace never
    shrinks."""
    chunk = 256 << 20
    with hip.Context(0, 1 << 20) as ctx:
        rec, facts = hrecord.ceiling_case(hrecord.MAX_TOTAL)
        total = facts["total"]
        n = total + 1 + GUARD
        d_rec = ctx.dmalloc(rec.size)
        d_out = ctx.dmalloc(n)
        try:
            ctx.to_device(d_rec, rec)
            ctx.to_device(d_out + total, np.full(n - total, FILL, np.uint8))
            size, lf, used = ctx.huffman_decode_device(d_rec, rec.size, d_out, total)
            assert size == total and used == rec.size and lf.tolist() == facts["lf"]
            st = _stats(ctx)
            assert st["runs"] == 3 and st["max_code_len"] >= 1
            back = np.empty(chunk, np.uint8)
            for lo in range(0, total, chunk):
                k = min(chunk, total - lo)
                assert ctx.lib.bwtc_hip_memcpy_to_host(ctx.handle, back.ctypes.data_as(ctypes.c_void_p),
                                                       ctypes.c_void_p(d_out + lo), k) == 0
                assert (back[:k] == hrecord.expected(facts, lo, lo + k)).all(), lo
            tail = np.empty(n - total, np.uint8)
            assert ctx.lib.bwtc_hip_memcpy_to_host(ctx.handle, tail.ctypes.data_as(ctypes.c_void_p),
                                                   ctypes.c_void_p(d_out + total), tail.size) == 0
            assert (tail == FILL).all(), "bytes after the block written"
            # one byte more: refused before anything is written (the buffer would hold it)
            rec1, facts1 = hrecord.ceiling_case(hrecord.MAX_TOTAL + 1)
            ctx.dfree(d_rec)
            d_rec = ctx.dmalloc(rec1.size)
            ctx.to_device(d_rec, rec1)
            with pytest.raises(hip.BwtcHipError) as e:
                ctx.huffman_decode_device(d_rec, rec1.size, d_out, facts1["total"])
            assert e.value.code == hip.E_CAPACITY
        finally:
            ctx.dfree(d_rec)
            ctx.dfree(d_out)


# ---- 7. exact error codes ------------------------------------------------------------------------------

def test_exact_error_codes(hip_ctx):
    good, good_facts = hrecord.code_shape_case(17)
    for name, code, rec, _ in hrecord.damaged_cases():
        rc, _ = _decode_guarded(hip_ctx, rec, 1 << 21)
        assert rc == getattr(hip, code), (name, rc, code)
        rc, got = _decode_guarded(hip_ctx, good, good_facts["total"])           # the context still decodes
        assert rc == 0 and (got == hrecord.expected(good_facts)).all(), name
    rc, _ = _decode_guarded(hip_ctx, good, good_facts["total"] - 1)
    assert rc == hip.E_CAPACITY


# ---- 8. foreign codes on real blocks, end to end -------------------------------------------------------

def _deep_recode(bwt, lf, oracle):
    """bwt's runs in the oracle's sections, every section coded with a complete depth-64 code over all 256
    symbols whose longest codes go to the most frequent run symbols."""
    freqs = np.bincount(bwt, minlength=256).astype(np.uint32)
    lengths = np.sort(hrecord.complete_code(64, 256))[::-1]
    secs = []
    for s, ln in blockgen.section_runs(bwt, oracle.oracle_sections(freqs)):
        order = np.argsort(-np.bincount(s, minlength=256), kind="stable")
        clen = np.zeros(256, np.int64)
        clen[order] = lengths
        secs.append((s, ln, clen))
    return hrecord.write_record(lf, secs)


def _uncompress_bin():
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwtc_amd", "host", "uncompress")


@pytest.mark.parametrize("kind", ["text_2M", "random_1M"])
def test_foreign_depth_64_codes_end_to_end(kind, hip_ctx, oracle, tmp_path):
    data = synth.gen_text(2 << 20, 3) if kind == "text_2M" else \
        np.random.default_rng(6).integers(0, 256, 1 << 20).astype(np.uint8)
    bwt, lf, _ = oracle.oracle_bwt_block(data, 8)
    rec, facts = _deep_recode(bwt, lf, oracle)
    assert max(s["h_M"] for s in facts["sections"]) == 64
    assert (hrecord.expected(facts) == bwt).all()
    stream = frame(b"H", rec.tobytes(), data.size)
    back = oracle.oracle_decompress_H(stream, data.size + 8)
    assert back is not None and (back == data).all()
    got, used = hip_ctx.decode_block_H(rec, with_consumed=True)
    assert used == rec.size and (got == data).all()
    assert _stats(hip_ctx)["max_code_len"] == 64
    src = tmp_path / "in.bwtc"
    src.write_bytes(stream.tobytes())
    for route in ("", "host"):
        env = dict(os.environ)
        env.pop("BWTC_HIP_DECODE", None)
        if route:
            env["BWTC_HIP_DECODE"] = route
        dst = tmp_path / ("out_%s.bin" % (route or "device"))
        subprocess.run([_uncompress_bin(), str(src), str(dst)], check=True, timeout=300, env=env)
        assert dst.read_bytes() == data.tobytes(), route or "device"
