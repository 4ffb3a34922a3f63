"""GPU tests of `uncompress` on 'B' / 'b' / 'u' files: the default route (host range decoder, wavelet rebuild and
inverse on the GPU) against BWTC_HIP_DECODE=host (the serial WaveletDecoder) and against the input, byte for byte,
with the debug tally proving which route every block took."""
import os
import re
import subprocess

import numpy as np
import pytest

from bwtc_amd import hip, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bwtc_amd", "host", "compress")
UNEXE = os.path.join(ROOT, "bwtc_amd", "host", "uncompress")


def _tally(stderr):
    m = re.search(r"^wavelet decode: device (\d+) host (\d+) ms_range_decode ([0-9.]+) ms_rebuild ([0-9.]+) ms_inverse ([0-9.]+) "
                  r"wall_ms ([0-9.]+)$", stderr, re.M)
    assert m, stderr
    return int(m.group(1)), int(m.group(2)), float(m.group(3)), float(m.group(4))


FLOOR = 64 << 10


def _packed(buf, pos):
    v, shift = 0, 0
    while True:
        b = int(buf[pos]); pos += 1
        v |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return v, pos


def _record_block_size(rec):
    """Bytes a record announces: 6-byte length, LF powers (a count byte, 31 bits each, byte padded), the sections' lengths."""
    n_lf = int(rec[6]) + 1
    pos = 6 + (8 + 31 * n_lf + 7) // 8
    sections = int(rec[pos]) or 256
    pos += 1
    total = 0
    for _ in range(sections):
        v, pos = _packed(rec, pos)
        total += v
    return total


def _expected_routes(stream):
    """(device, host) slices of a compressed file by the rule of Decompressor::decompress: a block with a grammar whose
    slices hold at least the floor between them stays on the device whole; any other slice goes by its own size."""
    stream = np.frombuffer(stream, np.uint8)
    pos, device, host = 1, 0, 0
    while True:
        original, pos = _packed(stream, pos)
        if original == 0:
            return device, host
        slices, pos = _packed(stream, pos)
        g = hip.Grammar()
        pos += g.read(stream[pos:])
        sizes = []
        for _ in range(slices):
            n = int.from_bytes(stream[pos:pos + 6].tobytes(), "big")
            sizes.append(_record_block_size(stream[pos:pos + 6 + n]))
            pos += 6 + n
        if g.rules > 0 and sum(sizes) >= FLOOR:
            device += len(sizes)
        else:
            device += sum(1 for v in sizes if v >= FLOOR)
            host += sum(1 for v in sizes if v < FLOOR)


@pytest.mark.parametrize("coder", ["B", "b", "u"])
@pytest.mark.parametrize("prepr", [None, "ppp"])
@pytest.mark.parametrize("blocks", [1, 4])
def test_uncompress_routes(tmp_path, coder, prepr, blocks):
    assert os.path.exists(EXE) and os.path.exists(UNEXE)
    # --mem 1 gives blocks of 740 000 bytes
    n = 600_000 if blocks == 1 else 2_700_000
    data = np.concatenate([synth.gen_text(n - 60_000, 3), synth.gen_random_bytes(40_000, 1), np.zeros(20_000, np.uint8)])
    src, dst = tmp_path / "input.bin", tmp_path / "input.bwtc"
    src.write_bytes(data.tobytes())
    cmd = [EXE, "-m", "1", "-s", "8", "-e", coder] + (["--prepr", prepr] if prepr else []) + [str(src), str(dst)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(name, **env):
        out = tmp_path / name
        r = subprocess.run([UNEXE, str(dst), str(out)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, BWTC_HIP_DEBUG="1", **env))
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == data.tobytes(), name
        return _tally(r.stderr)

    # every slice at or above the 64 KiB floor goes through the device and no other: the numbers come from the file itself
    want_device, want_host = _expected_routes(dst.read_bytes())
    assert want_device >= blocks
    device, host, ms_range, ms_rebuild = run("default.bin")
    assert (device, host) == (want_device, want_host) and ms_range > 0 and ms_rebuild > 0, (device, host, want_device, want_host)
    device2, host2, _, _ = run("host.bin", BWTC_HIP_DECODE="host")
    assert (device2, host2) == (0, want_device + want_host), (device2, host2, want_device, want_host)


def test_small_blocks_stay_on_the_host(tmp_path):
    data = synth.gen_text(30_000, 3)
    src, dst, out = tmp_path / "s.bin", tmp_path / "s.bwtc", tmp_path / "s.out"
    src.write_bytes(data.tobytes())
    assert subprocess.run([EXE, "-s", "8", "-e", "B", str(src), str(dst)], capture_output=True, timeout=600).returncode == 0
    r = subprocess.run([UNEXE, str(dst), str(out)], capture_output=True, text=True, timeout=600, env=dict(os.environ, BWTC_HIP_DEBUG="1"))
    assert r.returncode == 0 and out.read_bytes() == data.tobytes(), r.stderr
    device, host, _, _ = _tally(r.stderr)
    assert device == 0 and host == 1
