"""GPU tests of the 'H' record decoder (bwtc_hip_huffman_decode / _device, bwtc_hip_decode_block_H).

Records are made by the oracle's encoder, so the encoder and the decoder under test do not vouch
for each other; transformed blocks and LF powers are compared with the oracle's transform, and the
final bytes with the input."""
import ctypes
import json
import os

import numpy as np
import pytest

from bwtc_amd import hip, synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _packed(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _inputs():
    rng = np.random.default_rng(2024)
    yield "abracadabra", np.frombuffer(b"abracadabra", np.uint8), 1
    yield "one_byte", np.frombuffer(b"x", np.uint8), 1
    yield "all_equal", np.full(70001, 7, np.uint8), 8
    yield "two_syms", np.tile(np.array([0, 255], np.uint8), 30000), 8
    yield "random_64k", rng.integers(0, 256, 65536).astype(np.uint8), 8
    yield "random_300k", rng.integers(0, 256, 300000).astype(np.uint8), 3
    yield "uniform_3M_256_sections", rng.integers(0, 256, 3 << 20).astype(np.uint8), 8
    yield "text_1M", synth.gen_text(1 << 20, 3), 8
    yield "dna_1M", synth.gen_dna(1 << 20, 2), 8
    yield "long_runs", np.repeat(rng.integers(0, 4, 3000).astype(np.uint8), rng.integers(1, 5000, 3000)), 8
    yield "skew", (rng.geometric(0.3, 500000) % 256).astype(np.uint8), 16


def _freqs(bwt):
    return np.bincount(bwt, minlength=256).astype(np.uint32)


def _device_route(ctx, runs=None):
    st = ctx.huffman_decode_stats()
    assert st["route"] == 1 and st["tiles"] > 0 or st["runs"] == 0, st
    if runs is not None:
        assert st["runs"] == runs, st
    return st


def test_inputs_decode_to_oracle_bwt_and_input(hip_ctx, oracle):
    for name, data, sp in _inputs():
        bwt, lf, freqs = oracle.oracle_bwt_block(data, sp)
        rec = oracle.oracle_huffman_encode_block(bwt, lf, freqs)
        tail = np.concatenate([rec, np.full(37, 0xC3, np.uint8)])      # a record may be followed by more bytes
        got, glf, used = hip_ctx.huffman_decode(tail)
        assert used == rec.size, name
        assert got.tobytes() == bwt.tobytes(), name
        assert glf.tolist() == list(lf), name
        _device_route(hip_ctx)
        back, used2 = hip_ctx.decode_block_H(rec, with_consumed=True)
        assert used2 == rec.size and back.tobytes() == data.tobytes(), name
        st = _device_route(hip_ctx)
        assert st["sections"] >= 1 and st["host_syncs"] == st["sections"], (name, st)


def _entropy_roundtrip(hip_ctx, oracle, bwt, lf=(0,)):
    bwt = np.ascontiguousarray(bwt, np.uint8)
    lf = np.array(lf, np.uint32)
    rec = oracle.oracle_huffman_encode_block(bwt, lf, _freqs(bwt))
    got, glf, used = hip_ctx.huffman_decode(rec)
    assert used == rec.size
    assert got.size == bwt.size and got.tobytes() == bwt.tobytes()
    assert glf.tolist() == lf.tolist()
    return _device_route(hip_ctx)


def test_long_huffman_codes(hip_ctx, oracle):
    # Fibonacci-like run frequencies: the rarest symbols get codes far longer than 12 bits
    fib = [1, 1]
    while len(fib) < 27:
        fib.append(fib[-1] + fib[-2])
    syms = np.concatenate([np.full(f, k * 7 % 256, np.uint8) for k, f in enumerate(fib)])
    rng = np.random.default_rng(5)
    rng.shuffle(syms)
    st = _entropy_roundtrip(hip_ctx, oracle, syms)
    assert st["max_code_len"] > 12, st                  # the first-code / offset per length path ran


def test_single_symbol_and_empty_sections(hip_ctx, oracle):
    _entropy_roundtrip(hip_ctx, oracle, np.full(5000, 42, np.uint8))          # one symbol, one run
    two = np.repeat(np.array([3, 200, 3, 200], np.uint8), [100, 7, 1, 9000])  # most sections empty
    _entropy_roundtrip(hip_ctx, oracle, two)


def test_gamma_fixed_length_codes(hip_ctx, oracle):
    rng = np.random.default_rng(9)
    # all runs of 1 byte: every gamma code is the 1-bit "1"
    a = rng.integers(0, 255, 400000).astype(np.uint8)
    a[1:][a[1:] == a[:-1]] = 255
    a[1:][a[1:] == a[:-1]] = 254
    r = np.concatenate([[True], a[1:] != a[:-1]])
    assert r.all()
    _entropy_roundtrip(hip_ctx, oracle, a)
    # all runs of 2 or 3 bytes: a fixed 3-bit gamma code
    syms = np.arange(200000, dtype=np.int64) % 251
    lens = rng.integers(2, 4, syms.size)
    _entropy_roundtrip(hip_ctx, oracle, np.repeat(syms.astype(np.uint8), lens))


def test_run_of_2_pow_26(hip_ctx, oracle):
    # one run of 2^26 bytes: a 53-bit gamma code
    _entropy_roundtrip(hip_ctx, oracle, np.full(1 << 26, 9, np.uint8), lf=(12345,))


def test_golden_reference_stream(hip_ctx):
    c = [x for x in json.load(open(os.path.join(G, "streams.json")))["cases"] if x["coder"] == "H"][0]
    data = np.frombuffer(c["input_ascii"].encode(), np.uint8)
    stream = bytes.fromhex(c["stream_hex"])
    head = b"H" + _packed(data.size) + _packed(1) + b"\x00"
    assert stream.startswith(head)
    rec = np.frombuffer(stream[len(head):], np.uint8)
    back, used = hip_ctx.decode_block_H(rec, with_consumed=True)
    assert back.tobytes() == data.tobytes()
    assert stream[len(head) + used:] == b"\x00"


@pytest.mark.parametrize("mib", [64, 256])
def test_product_records_large_text(mib):
    size = mib << 20
    data = synth.gen_text(size, 3)
    with hip.Context(0, size) as ctx:
        rec, bwt = ctx.transform_and_encode(data, 8)
        got, lf, used = ctx.huffman_decode(rec)
        assert used == rec.size and got.tobytes() == bwt.tobytes()
        st = _device_route(ctx)
        back = ctx.decode_block_H(rec)
        assert back.tobytes() == data.tobytes()
        st = _device_route(ctx)
        assert st["ms_entropy"] <= st["ms_entropy_wall"] + 1e-3
        print("%d MiB C3: entropy %.2f ms device / %.2f ms wall, inverse %.2f ms, %d sections, %d tiles, M %.2f"
              % (mib, st["ms_entropy"], st["ms_entropy_wall"], st["ms_inverse"], st["sections"], st["tiles"],
                 st["map_entries"] / st["tiles"]))


def test_record_followed_by_a_long_tail(oracle):
    """Only the record the 48-bit length announces is uploaded and mapped: the workspace does not
    grow with what follows it in the buffer (the rest of a file, say)."""
    data = synth.gen_text(1 << 20, 3)
    bwt, lf, freqs = oracle.oracle_bwt_block(data, 8)
    rec = oracle.oracle_huffman_encode_block(bwt, lf, freqs)
    tail = np.random.default_rng(4).integers(0, 256, 64 << 20).astype(np.uint8)
    ws = []
    for buf in (rec, np.concatenate([rec, tail])):
        with hip.Context(0, data.size) as ctx:
            got, glf, used = ctx.huffman_decode(buf)
            assert used == rec.size and got.tobytes() == bwt.tobytes()
            ws.append(ctx.huffman_decode_stats()["workspace_bytes"])
            back, used = ctx.decode_block_H(buf, with_consumed=True)
            assert used == rec.size and back.tobytes() == data.tobytes()
    assert ws[0] == ws[1], ws


def test_entropy_decode_beyond_context_block_size(oracle):
    # the entropy-only entry point needs no context workspace: cap is the limit, not max_block_size
    data = synth.gen_text(300000, 3)
    bwt, lf, freqs = oracle.oracle_bwt_block(data, 8)
    rec = oracle.oracle_huffman_encode_block(bwt, lf, freqs)
    with hip.Context(0, 1 << 16) as ctx:
        got, _, _ = ctx.huffman_decode(rec, cap=data.size)
        assert got.tobytes() == bwt.tobytes()
        with pytest.raises(hip.BwtcHipError) as e:
            ctx.decode_block_H(rec, cap=data.size)
        assert e.value.code == hip.E_CAPACITY


# ---- damaged records -----------------------------------------------------------------------------

GUARD = 4096


def _decode_guarded(ctx, rec, cap):
    """_device decode into a buffer with a guard region after `cap` bytes; returns (rc, bytes)."""
    rec = np.ascontiguousarray(rec, np.uint8)
    d_rec = ctx.dmalloc(max(rec.size, 1))
    d_out = ctx.dmalloc(cap + GUARD)
    try:
        if rec.size:
            ctx.to_device(d_rec, rec)
        guard = np.full(cap + GUARD, 0xE7, np.uint8)
        ctx.to_device(d_out, guard)
        lf = np.zeros(256, np.uint32)
        n_lf, size, used = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
        rc = ctx.lib.bwtc_hip_huffman_decode_device(ctx.handle, ctypes.c_void_p(d_rec), rec.size, ctypes.c_void_p(d_out),
                                                    cap, lf.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_lf),
                                                    ctypes.byref(size), ctypes.byref(used))
        back = np.empty(cap + GUARD, np.uint8)
        assert ctx.lib.bwtc_hip_memcpy_to_host(ctx.handle, back.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_out),
                                               back.size) == 0
        assert (back[cap:] == 0xE7).all(), "guard region written"
        if rc == 0:
            assert size.value <= cap
        return rc, back[:size.value] if rc == 0 else None
    finally:
        ctx.dfree(d_rec)
        ctx.dfree(d_out)


def test_damaged_records(hip_ctx, oracle):
    rng = np.random.default_rng(77)
    data = np.concatenate([synth.gen_text(200000, 3), rng.integers(0, 256, 100000).astype(np.uint8)])
    bwt, lf, freqs = oracle.oracle_bwt_block(data, 8)
    rec = oracle.oracle_huffman_encode_block(bwt, lf, freqs)
    cap = data.size + 100
    rc, got = _decode_guarded(hip_ctx, rec, cap)
    assert rc == 0 and got.tobytes() == bwt.tobytes()
    codes = []
    # truncated
    for k in (0, 3, 7, 20, 60, rec.size // 3, rec.size // 2, rec.size - 40, rec.size - 1):
        rc, _ = _decode_guarded(hip_ctx, rec[:k], cap)
        assert rc < 0, k
        codes.append(rc)
    assert hip.E_PAST_RECORD in codes
    # wrong 48-bit length field
    bad = rec.copy()
    bad[5] ^= 0x04
    rc, _ = _decode_guarded(hip_ctx, bad, cap)
    assert rc == hip.E_LENGTH
    # block above the capacity
    rc, _ = _decode_guarded(hip_ctx, rec, data.size - 1)
    assert rc == hip.E_CAPACITY
    # flipped bits everywhere: in the header, shapes, Huffman and gamma streams
    for pos in list(range(6, 80, 3)) + [int(x) for x in rng.integers(80, rec.size, 60)]:
        bad = rec.copy()
        bad[pos] ^= np.uint8(1 << int(rng.integers(0, 8)))
        rc, got = _decode_guarded(hip_ctx, bad, cap)
        assert rc == 0 or rc in (hip.E_NO_CODE, hip.E_SHAPE, hip.E_PAST_RECORD, hip.E_RUNS, hip.E_CAPACITY,
                                 hip.E_LENGTH), (pos, rc)
    # the context still decodes a good record
    got, glf, used = hip_ctx.huffman_decode(rec)
    assert got.tobytes() == bwt.tobytes() and used == rec.size
    assert hip_ctx.decode_block_H(rec).tobytes() == data.tobytes()


# ---- CLI -----------------------------------------------------------------------------------------

def _bin(name):
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwtc_amd", "host", name)


@pytest.mark.parametrize("extra", [[], ["--prepr", "p"]])
def test_cli_device_and_host_routes(tmp_path, extra):
    import subprocess
    rng = np.random.default_rng(3)
    data = np.concatenate([synth.gen_text(1 << 20, 3), rng.integers(0, 256, 300000).astype(np.uint8),
                           synth.gen_dna(500000, 2)])
    src = tmp_path / "in.bin"
    src.write_bytes(data.tobytes())
    comp = tmp_path / "in.bwtc"
    subprocess.run([_bin("compress"), "-m", "4", "-e", "H"] + extra + [str(src), str(comp)], check=True, timeout=300)
    outs = []
    for route in ("", "host"):
        env = dict(os.environ)
        env.pop("BWTC_HIP_DECODE", None)
        if route:
            env["BWTC_HIP_DECODE"] = route
        dst = tmp_path / ("out_%s.bin" % (route or "device"))
        subprocess.run([_bin("uncompress"), str(comp), str(dst)], check=True, timeout=300, env=env)
        outs.append(dst.read_bytes())
    assert outs[0] == data.tobytes()
    assert outs[1] == data.tobytes()
    assert outs[0] == outs[1]
