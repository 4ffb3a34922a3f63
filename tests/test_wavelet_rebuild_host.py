"""CPU tests of the wavelet rebuild's host side: the library's host half of the 'B' / 'b' / 'u' decoders (range
decoder into a flattened forest) and bwtc_hip_host_wavelet_rebuild, the host twin of the rebuild kernels.

The forests of tests/wforest.py are written the way the encoder fills the nodes, so the expected bytes are the runs
themselves; streams come from the oracle's encoder and are held against the oracle's transform."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import wforest
from bwtc_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRANULARITIES = (1, 2, 7, 8, 64, 1000)


def test_builder_and_library_against_the_oracle(oracle):
    """Oracle streams of every letter, one block and several through ONE handle, decode to the oracle's transformed
    bytes and LF powers; the builder's framing reads every record to its end."""
    for letter in "Bbu":
        for name, data in wforest.decoder_inputs():
            for bs, sp in ((data.size, 8), (data.size // 3 + 1, 4)):
                stream = oracle.oracle_compress_wavelet(letter, data, bs, sp)
                coder, recs = wforest.records(stream)
                assert coder == letter and sum(n for n, _ in recs) == data.size
                dec, counter = hip.WaveletDecoder(letter), hip.WaveletDecoder(letter)
                off = 0
                for n, rec in recs:
                    bwt, lf, _ = oracle.oracle_bwt_block(data[off:off + n], sp)
                    tail = np.concatenate([rec, np.full(11, 0xC3, np.uint8)])
                    got, glf, used = dec.decode_bwt_host(tail, n)
                    assert used == rec.size, (letter, name, off)
                    assert got.tobytes() == bwt.tobytes(), (letter, name, off)
                    assert glf.tolist() == list(lf), (letter, name, off)
                    c, used2 = counter.counts(rec, n)
                    assert used2 == rec.size and c["bytes"] == n and 1 <= c["runs"] <= n and c["sections"] >= 1, c
                    off += n


def test_library_equals_wavelet_decoder_program(oracle):
    """tests/cpp/wavelet_rebuild_test.cpp: the same streams through the host mirror's WaveletDecoder and the library,
    byte for byte, consumed lengths included; cut and damaged records end in return codes."""
    exe = os.path.join(ROOT, "tests", "cpp", "wavelet_rebuild_test")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "bwtc_amd", "host"), "../../tests/cpp/wavelet_rebuild_test"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all tests passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("name", sorted(wforest.cases()))
def test_hand_built_forests(name):
    sections, gap = wforest.cases()[name]
    forest, runs, reads = wforest.pack(sections, gap)
    want = wforest.expand(runs)
    for g in GRANULARITIES:
        got, got_reads = hip.host_wavelet_rebuild(forest, line_words=g)
        assert got.size == want.size and got.tobytes() == want.tobytes(), (name, g)
        assert got_reads == reads, (name, g)


def test_run_of_2_pow_31_minus_1():
    """The longest run the route takes: W = 15 and sixteen leading ones."""
    n = (1 << 31) - 1
    assert wforest.escape_bits(n, 15).startswith("1" * 16 + "0")
    forest, runs, reads = wforest.pack([wforest.section([(200, n)], W=15)])
    out = np.empty(n + 64, np.uint8)
    out[n:] = 0xA5
    size, got_reads = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = hip.load().bwtc_hip_host_wavelet_rebuild(ctypes.byref(forest.c), out.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(size), 7,
                                                  ctypes.byref(got_reads))
    assert rc == 0 and size.value == n and got_reads.value == reads
    for a in range(0, n, 1 << 28):
        assert (out[a:min(n, a + (1 << 28))] == 200).all()
    assert (out[n:] == 0xA5).all()
    # one byte more is beyond the route
    forest2, _, _ = wforest.pack([wforest.section([(200, n), (3, 1)], W=15)])
    rc = hip.load().bwtc_hip_host_wavelet_rebuild(ctypes.byref(forest2.c), out.ctypes.data_as(ctypes.c_void_p), n + 1, ctypes.byref(size), 7, None)
    assert rc == hip.E_W_LIMIT


@pytest.mark.parametrize("name", sorted(wforest.corrupt_cases()))
def test_corrupt_forests_return_their_code_and_write_nothing_past_cap(name):
    forest, cap, code = wforest.corrupt_cases()[name]
    for g in GRANULARITIES:
        with pytest.raises(hip.BwtcHipError) as e:
            hip.host_wavelet_rebuild(forest, cap=cap, line_words=g)       # the wrapper checks the bytes past cap itself
        assert e.value.code == code, (name, g, e.value.code)


def test_decode_entry_points_are_exported():
    lib = hip.load()
    for name in ("bwtc_hip_decode_block_W", "bwtc_hip_decode_block_W_device"):
        assert hasattr(lib, name), name
    assert lib.bwtc_hip_decode_block_W(None, None, None, 0, None, 0, None, None) == -1      # no device needed


def test_bad_arguments():
    forest, _, _ = wforest.pack(wforest.cases()["single_symbol"][0])
    with pytest.raises(hip.BwtcHipError):
        hip.host_wavelet_rebuild(forest, line_words=0)
    with pytest.raises(hip.BwtcHipError):
        hip.WaveletDecoder("H")
