"""`compress` under BWTC_HIP_BATCH (-m gpu): the stream of a batched run must be the stream of the plain run and the
oracle's, byte for byte, for 'H', 'B' and 'b'; `uncompress` gives the input back.  -m 1 cuts 3 000 000 bytes into
sixteen blocks of 185 000 bytes and one of 40 000: with sixteen blocks to a batch the last batch holds one block,
and that block is short.

Without the feature the debug line that proves the batched route is missing."""
import os
import re
import subprocess

import numpy as np
import pytest

from bwtc_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bwtc_amd", "host", "compress")
UNEXE = os.path.join(ROOT, "bwtc_amd", "host", "uncompress")
BLOCK = 185_000
SIZE = 3_000_000


@pytest.fixture(scope="module")
def data():
    d = np.concatenate([synth.gen_text(SIZE - 400_000, 6), synth.gen_random_bytes(200_000, 2), np.zeros(100_000, np.uint8),
                        synth.gen_text(100_000, 7)])
    assert d.size == SIZE and SIZE // BLOCK == 16 and 0 < SIZE % BLOCK < BLOCK
    return d


@pytest.mark.parametrize("coder", ["H", "B", "b"])
def test_batched_stream_is_the_plain_stream(tmp_path, oracle, data, coder):
    assert os.path.exists(EXE) and os.path.exists(UNEXE)
    src = tmp_path / "in.bin"
    src.write_bytes(data.tobytes())
    env = {k: v for k, v in os.environ.items() if not k.startswith("BWTC_HIP_BATCH")}

    def run(name, **extra):
        dst = tmp_path / name
        r = subprocess.run([EXE, "-m", "1", "-s", "8", "-e", coder, str(src), str(dst)], capture_output=True, text=True, timeout=300,
                           env=dict(env, BWTC_HIP_DEBUG="1", **extra))
        assert r.returncode == 0, r.stderr
        return dst, r.stderr

    plain, plain_err = run("plain.bwtc")
    batched, batched_err = run("batched.bwtc", BWTC_HIP_BATCH="16")
    assert "batched transform" not in plain_err
    m = re.search(r"^batched transform: (\d+) blocks in (\d+) calls of up to (\d+)$", batched_err, re.M)
    assert m and [int(g) for g in m.groups()] == [17, 2, 16], batched_err
    # a block size above BWTC_HIP_BATCH_BLOCK: the stream is not batched
    _, small_err = run("limited.bwtc", BWTC_HIP_BATCH="16", BWTC_HIP_BATCH_BLOCK=str(BLOCK - 1))
    assert "batched transform" not in small_err
    want = oracle.oracle_compress_H(data, BLOCK, 8) if coder == "H" else oracle.oracle_compress_wavelet(coder, data, BLOCK, 8)
    assert batched.read_bytes() == plain.read_bytes()
    assert batched.read_bytes() == want.tobytes()
    out = tmp_path / "back.bin"
    r = subprocess.run([UNEXE, str(batched), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == data.tobytes()
