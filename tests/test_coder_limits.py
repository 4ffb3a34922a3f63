"""The limit cases of the entropy coders (tests/blockgen.py limit_blocks: Huffman depth 33, one run of
64 MiB, runs of 2^16..2^25 bytes, 74 000 long runs, section starts inside runs at tile edges, a section
of > 65 536 dense ids) on the CPU: every case still reaches the edge it is built for, and the oracle's
own 'H' and 'B' encoders decode back to the block -- the oracle is what the device kernels are held to
at these edges (tests/test_gpu_coder_limits.py), and nothing else checks it there."""
import numpy as np
import pytest

import blockgen


def _packed(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def frame(coder, record, size):
    """Compressor::compress framing of one block: coder letter, one precompressor block, no grammar."""
    return np.frombuffer(coder + _packed(size) + _packed(1) + b"\x00" + record + b"\x00", np.uint8)


@pytest.mark.parametrize("name", blockgen.LIMIT_CASE_NAMES)
def test_limit_case_reaches_its_edge_and_the_oracle_decodes_it_back(name, oracle):
    [(_, block, edge)] = list(blockgen.limit_blocks(names=(name,)))
    assert block.size <= (64 << 20) + 1024                  # one block of the GPU tests' context
    m = blockgen.limit_measures(block, oracle)
    for measure, least in edge.items():
        assert m[measure] >= least, (name, measure, m[measure], least, m)
    lf = np.zeros(1, np.uint32)
    freqs = np.bincount(block, minlength=256).astype(np.uint32)
    rec = oracle.oracle_huffman_encode_block(block, lf, freqs)
    back = oracle.oracle_decode_transformed("H", frame(b"H", rec.tobytes(), block.size), block.size + 8)
    assert back is not None and back.size == block.size and (back == block).all(), ("H", name)
    rec = oracle.oracle_wavelet_encode_block(block, lf, freqs)
    back = oracle.oracle_decode_transformed("B", frame(b"B", rec.tobytes(), block.size), block.size + 8)
    assert back is not None and back.size == block.size and (back == block).all(), ("B", name)

