"""GPU tests of the C++ host mirror (bwtc_amd/host): the C++ test program shaped after the
reference's InverseBwtTest / LFpowersTest / CompressorAndDecompressorTest, and the `compress`
command line tool, whose output must decode (here: with the oracle's decoder) to the input."""
import os
import subprocess

import numpy as np
import pytest

from bwtc_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG = dict(os.environ, BWTC_HIP_DEBUG="1")


def _routes(stderr):
    """The `bwtc_hip routes: ...` line compress prints at exit under BWTC_HIP_DEBUG (the wavelet
    routes of all its contexts, summed), as a dict."""
    lines = [ln for ln in stderr.splitlines() if ln.startswith("bwtc_hip routes: ")]
    assert len(lines) == 1, stderr[-2000:]
    return {k: int(v) for k, v in (f.split("=") for f in lines[0].split(": ", 1)[1].split())}


def _assert_no_rejection(r):
    assert r["models_rejected"] == 0 and r["reject_reasons"] == 0, r
    assert r["trees_device"] > 0 and r["models_device"] > 0, r


def test_cpp_host_mirror_program():
    exe = os.path.join(ROOT, "tests", "cpp", "host_mirror_test")
    assert os.path.exists(exe), "build with __graft_entry__.build() / make -C bwtc_amd/host"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "all tests passed" in r.stdout


def test_compress_cli_roundtrip(tmp_path, oracle):
    exe = os.path.join(ROOT, "bwtc_amd", "host", "compress")
    assert os.path.exists(exe)
    data = np.concatenate([synth.gen_text(3_000_000, 3), synth.gen_random_bytes(500_000, 1),
                           np.zeros(100_000, np.uint8)])
    src = tmp_path / "input.bin"
    dst = tmp_path / "input.bin.bwtc"
    src.write_bytes(data.tobytes())
    # --mem 10 -> BWT blocks of 1.85 MB -> two blocks
    r = subprocess.run([exe, "-m", "10", "-s", "8", "--bwt", "g", "-e", "H", "-v", "1", str(src), str(dst)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    stream = np.frombuffer(dst.read_bytes(), np.uint8)
    assert stream[0] == ord("H")
    back = oracle.oracle_decompress_H(stream, data.size + 8)
    assert back is not None and back.tobytes() == data.tobytes()
    assert stream.tobytes() == oracle.oracle_compress_H(data, int(10 * 1000000 * 0.185), 8).tobytes()
    # and back through this repository's own uncompress (host 'H' decoder + GPU inverse BWT)
    unexe = os.path.join(ROOT, "bwtc_amd", "host", "uncompress")
    out = tmp_path / "roundtrip.bin"
    r = subprocess.run([unexe, "-v", "1", str(dst), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == data.tobytes()
    # the reference's default coder 'B' (no -e): five blocks, overlapped by the Compressor loop
    dstb = tmp_path / "input.B.bwtc"
    r = subprocess.run([exe, "-m", "4", "-s", "8", "-v", "1", str(src), str(dstb)],
                       capture_output=True, text=True, timeout=600, env=DEBUG)
    assert r.returncode == 0, r.stderr
    routes = _routes(r.stderr)
    _assert_no_rejection(routes)
    assert routes["models_device"] == routes["trees_device"] and routes["lost_turn"] == 0, routes
    sb = dstb.read_bytes()
    assert sb[:1] == b"B"
    assert sb == oracle.oracle_compress_B(data, int(4 * 1000000 * 0.185), 8).tobytes()
    outb = tmp_path / "roundtrip.B.bin"
    r = subprocess.run([unexe, "-v", "1", str(dstb), str(outb)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert outb.read_bytes() == data.tobytes()
    # another model letter through both tools
    dstu = tmp_path / "input.u.bwtc"
    outu = tmp_path / "roundtrip.u.bin"
    r = subprocess.run([exe, "-m", "10", "-e", "u", str(src), str(dstu)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert dstu.read_bytes() == oracle.oracle_compress_wavelet("u", data, int(10 * 1000000 * 0.185), 8).tobytes()
    r = subprocess.run([unexe, str(dstu), str(outu)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert outu.read_bytes() == data.tobytes()
    r = subprocess.run([exe, "-e", "m", str(src), str(dstu)], capture_output=True, text=True)
    assert r.returncode != 0
    # rejected choices, as the reference's validators do (compress.cpp:86-96)
    r = subprocess.run([exe, "--bwt", "d", str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode != 0


def test_cli_block_farm_over_two_contexts_gives_the_sequential_stream(tmp_path, oracle):
    """`compress --devices 0,0` (bwtc_hip_farm.hpp: one thread + context + page-locked staging ring
    per entry, in-order writer, the 'B' coder's carried model state handed from context to context
    at bwtc_hip_wavelet_encode_queue): the stream must be byte-equal to the one-device stream and
    to the oracle's sequential encoder, for both coders, with more blocks than contexts."""
    exe = os.path.join(ROOT, "bwtc_amd", "host", "compress")
    unexe = os.path.join(ROOT, "bwtc_amd", "host", "uncompress")
    data = np.concatenate([synth.gen_text(5_300_000, 41), synth.gen_dna(1_000_000, 7), synth.gen_text(2_100_000, 43)])
    src = tmp_path / "farm.bin"
    src.write_bytes(data.tobytes())
    block = int(1 * 1000000 * 0.185)                  # -m 1 -> 185 000-byte blocks: 46 blocks
    for enc in ("B", "H"):
        one = tmp_path / ("one.%s.bwtc" % enc)
        for devices, dst in (("0,0", tmp_path / ("two.%s.bwtc" % enc)), ("0,0,0", tmp_path / ("three.%s.bwtc" % enc))):
            r = subprocess.run([exe, "-m", "1", "-e", enc, "--devices", devices, str(src), str(dst)],
                               capture_output=True, text=True, timeout=600, env=DEBUG)
            assert r.returncode == 0, r.stderr
            if enc == "B":
                _assert_no_rejection(_routes(r.stderr))
        r = subprocess.run([exe, "-m", "1", "-e", enc, str(src), str(one)], capture_output=True, text=True, timeout=600,
                           env=DEBUG)
        assert r.returncode == 0, r.stderr
        if enc == "B":
            _assert_no_rejection(_routes(r.stderr))
        want = (oracle.oracle_compress_B if enc == "B" else oracle.oracle_compress_H)(data, block, 8).tobytes()
        assert one.read_bytes() == want, enc
        assert (tmp_path / ("two.%s.bwtc" % enc)).read_bytes() == want, enc
        assert (tmp_path / ("three.%s.bwtc" % enc)).read_bytes() == want, enc
    # the 'B' models of a farmed stream run on the device (the state-dependent passes at _queue time,
    # the block joins the host pipeline from a stream callback): the same stream with the models on the
    # worker threads, and when every block's device result is declared flagged (host fallback)
    for extra in ({"BWTC_HIP_MODELS": "host"}, {"BWTC_HIP_TEST_MODELS_FALLBACK": "1"}):
        dst = tmp_path / "two.B.alt.bwtc"
        r = subprocess.run([exe, "-m", "1", "-e", "B", "--devices", "0,0", str(src), str(dst)],
                           capture_output=True, text=True, timeout=600, env=dict(DEBUG, **extra))
        assert r.returncode == 0, r.stderr
        assert dst.read_bytes() == (tmp_path / "two.B.bwtc").read_bytes(), extra
        routes = _routes(r.stderr)
        assert routes["models_device"] == 0, (extra, routes)
        if "BWTC_HIP_TEST_MODELS_FALLBACK" in extra:
            # every block whose passes ran on the device was turned down, for the test switch alone
            assert routes["models_rejected"] > 0 and routes["reject_reasons"] == 16, routes
            assert "the device models of a block were not used" in r.stderr
        else:
            assert routes["models_rejected"] == 0, routes
    out = tmp_path / "farm.out"
    r = subprocess.run([unexe, str(tmp_path / "two.B.bwtc"), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == data.tobytes()


def test_cli_roundtrip_full_size_block_default_coder(tmp_path):
    """BASELINE's configuration end to end: one 256 MiB text block, the default 'B' coder,
    compress -> uncompress (host wavelet decoder + GPU inverse BWT) gives the input back.
    Size-independent property; no oracle involved."""
    exe = os.path.join(ROOT, "bwtc_amd", "host", "compress")
    unexe = os.path.join(ROOT, "bwtc_amd", "host", "uncompress")
    data = synth.gen_text(256 << 20, 3)
    src = tmp_path / "text256.bin"
    dst = tmp_path / "text256.bwtc"
    out = tmp_path / "text256.out"
    src.write_bytes(data.tobytes())
    # --mem 1452 -> BWT block 0.185 * 1452e6 = 268.6 MB >= 256 MiB: one block
    r = subprocess.run([exe, "-m", "1452", "-s", "8", "-v", "1", str(src), str(dst)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    packed = dst.stat().st_size
    assert 40_000_000 < packed < 60_000_000, packed
    r = subprocess.run([unexe, "-v", "1", str(dst), str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    back = np.fromfile(out, np.uint8)
    assert back.size == data.size and (back == data).all()
    # three blocks (two full, one partial) overlapped by the Compressor loop, model state carried
    # across the block borders, decoded by one decoder object
    for f in (src, dst, out):
        f.unlink()
    data = np.concatenate([data, synth.gen_text(300 << 20, 31)])
    src.write_bytes(data.tobytes())
    r = subprocess.run([exe, "-m", "1452", "-s", "8", str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([unexe, str(dst), str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    back = np.fromfile(out, np.uint8)
    assert back.size == data.size and (back == data).all()


def test_cli_roundtrip_1GiB_single_block_default_coder(tmp_path):
    """The largest block the format carries (1 GiB, N = 2^30 + 1) through the default coder:
    2.2 billion steps in the stream kernels, one serial decoder pass, GPU inverse transform."""
    exe = os.path.join(ROOT, "bwtc_amd", "host", "compress")
    unexe = os.path.join(ROOT, "bwtc_amd", "host", "uncompress")
    data = synth.gen_text(1 << 30, 5)
    src = tmp_path / "t1g.bin"
    dst = tmp_path / "t1g.bwtc"
    out = tmp_path / "t1g.out"
    data.tofile(src)
    r = subprocess.run([exe, "-m", "5806", "-v", "1", str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    assert "outside the stream kernels" not in r.stderr          # the device route took it
    r = subprocess.run([unexe, str(dst), str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    back = np.fromfile(out, np.uint8)
    assert back.size == data.size and (back == data).all()


def _real_text(limit):
    """Real (not generated) text: the file BWTC_CORPUS names when there is one (SURVEY.md 8(d):
    enwik8 / enwik9), else tests/golden/real_text.txt.xz, a fixed 1.1 MB snapshot of the project's
    own documentation and sources -- anything written by people, so that the coders also see inputs
    that the 64-token generator never makes (other section sizes, other run statistics).
    Returns (text, its name, the `compress -m` that cuts it into several blocks)."""
    path = os.environ.get("BWTC_CORPUS")
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            return f.read(limit), os.path.basename(path), 50
    import lzma
    with lzma.open(os.path.join(ROOT, "tests", "golden", "real_text.txt.xz")) as f:
        return f.read(limit), "tests/golden/real_text.txt.xz", 2


def test_real_text_roundtrip_and_oracle_parity(tmp_path, oracle):
    """BWTC_CORPUS (or the stored real text) through `compress` (default coder 'B', models on the
    GPU) and `uncompress`, several blocks; the stream is also the oracle's, byte for byte."""
    data, name, mem = _real_text(24 << 20)
    assert len(data) >= (1 << 20), "less than 1 MiB of real text in %s" % name
    src = tmp_path / "corpus.bin"
    dst = tmp_path / "corpus.bwtc"
    out = tmp_path / "corpus.out"
    src.write_bytes(data)
    exe = os.path.join(ROOT, "bwtc_amd", "host", "compress")
    unexe = os.path.join(ROOT, "bwtc_amd", "host", "uncompress")
    r = subprocess.run([exe, "-m", str(mem), "-v", "1", str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    stream = dst.read_bytes()
    arr = np.frombuffer(data, np.uint8)
    assert stream == oracle.oracle_compress_B(arr, int(mem * 1000000 * 0.185), 8).tobytes(), name
    r = subprocess.run([unexe, str(dst), str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == data
    print("real text (%s): %d -> %d bytes, ratio %.3f" % (name, len(data), len(stream), len(stream) / len(data)))
