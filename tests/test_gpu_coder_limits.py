"""The device kernels of the 'H' and 'B' coders at their run, code and table limits (tests/blockgen.py
limit_blocks; tests/test_coder_limits.py checks that every case reaches its edge and that the oracle
decodes its own records back): run statistics section by section, the whole 'H' record and the whole
'B' record against the oracle, with the route counters showing that the device built the 'B' streams.
Also device-resident blocks at unaligned addresses, the 'b' and 'u' model letters, and the section of
more than 65 536 dense ids that takes the step sort out of the segmented layout."""
import re

import numpy as np
import pytest

import blockgen
from test_gpu_encode import _assert_device_models

pytestmark = pytest.mark.gpu
LF = np.zeros(1, np.uint32)


class _Limits:
    """Each case's block and the oracle's records of it, worked out once per module."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.cases = {}

    def __getitem__(self, name):
        if name not in self.cases:
            [(_, block, _)] = list(blockgen.limit_blocks(names=(name,)))
            freqs = np.bincount(block, minlength=256).astype(np.uint32)
            self.cases[name] = {
                "block": block, "freqs": freqs,
                "H": self.oracle.oracle_huffman_encode_block(block, LF, freqs).tobytes(),
                "B": self.oracle.oracle_wavelet_encode_block(block, LF, freqs).tobytes()}
        return self.cases[name]


@pytest.fixture(scope="module")
def limits(oracle):
    return _Limits(oracle)


@pytest.mark.parametrize("name", blockgen.LIMIT_CASE_NAMES)
def test_limit_run_statistics_match_oracle(name, hip_ctx, oracle, limits):
    """wavelet_section_stats_device (run scanners, the dense table, the overflow list and its second
    copy, the sorted lengths of 2^20 and more) against utils::calculateRunsAndCharacters per section."""
    c = limits[name]
    block = c["block"]
    sec, rf, tot, dist = hip_ctx.wavelet_section_stats(block, c["freqs"])
    assert (sec == oracle.oracle_sections(c["freqs"])).all(), name
    beg = 0
    for s in range(sec.size):
        orf, oruns, odist = oracle.oracle_runs_and_characters(block[beg:beg + int(sec[s])])
        assert (rf[s].astype(np.uint64) == orf).all(), (name, s)
        assert int(tot[s]) == oruns, (name, s, int(tot[s]), oruns)
        assert dist[s] == odist, (name, s)
        beg += int(sec[s])


@pytest.mark.parametrize("name", blockgen.LIMIT_CASE_NAMES)
def test_limit_huffman_record_matches_oracle(name, hip_ctx, limits):
    c = limits[name]
    got = hip_ctx.huffman_encode(c["block"], LF, c["freqs"])
    assert got.size == len(c["H"]), (name, got.size, len(c["H"]))
    assert got.tobytes() == c["H"], name


@pytest.mark.parametrize("name", blockgen.LIMIT_CASE_NAMES)
def test_limit_wavelet_record_matches_oracle(name, hip_ctx, limits):
    c = limits[name]
    hip_ctx.wavelet_reset()
    hip_ctx.wavelet_routes(reset=True)
    got = hip_ctx.wavelet_encode(c["block"], LF, c["freqs"], threads=4)
    r = hip_ctx.wavelet_routes()
    assert got.size == len(c["B"]), (name, got.size, len(c["B"]))
    assert got.tobytes() == c["B"], name
    _assert_device_models(r, blocks=1)


def test_limit_many_ids_leave_the_segmented_layout(hip_ctx, limits, capfd, monkeypatch):
    """A section of 256 symbol leaves and some 1200 integer nodes has far more than 65 536 dense ids:
    the step sort leaves the segmented layout (BWTC_HIP_DEBUG_SEG reports each section it weighs)."""
    c = limits["many_ids"]
    monkeypatch.setenv("BWTC_HIP_DEBUG_SEG", "1")
    capfd.readouterr()
    hip_ctx.wavelet_reset()
    hip_ctx.wavelet_routes(reset=True)
    got = hip_ctx.wavelet_encode(c["block"], LF, c["freqs"], threads=4)
    err = capfd.readouterr().err
    assert got.tobytes() == c["B"]
    _assert_device_models(hip_ctx.wavelet_routes(), blocks=1)
    seen = [tuple(int(x) for x in m) for m in
            re.findall(r"section (\d+): (\d+) groups, (\d+) symbol nodes, (\d+) leaves -> (\d+) ids", err)]
    assert seen, err[-2000:]
    s, groups, nodes, leaves, ids = seen[-1]           # the loop stops at the first section over the limit
    assert s == 0 and leaves == 256 and ids > 65536, seen[-3:]
    print("many_ids: section 0 has %d groups, %d symbol nodes, %d leaves -> %d ids" % (groups, nodes, leaves, ids))


@pytest.mark.parametrize("name", ["fib_depth", "sections_inside_runs"])
@pytest.mark.parametrize("offset", [1, 7])
def test_limit_device_blocks_at_unaligned_addresses(name, offset, hip_ctx, limits):
    """huffman_encode_device / wavelet_encode_device on a block that starts `offset` bytes past an
    allocation: the run scanners' unaligned path."""
    c = limits[name]
    block = c["block"]
    cap = hip_ctx.compress_bound(block.size)
    d_in = hip_ctx.dmalloc(block.size + 16)
    d_out = hip_ctx.dmalloc(cap)
    try:
        hip_ctx.to_device(d_in + offset, block)
        n = hip_ctx.huffman_encode_device(d_in + offset, block.size, LF, c["freqs"], d_out, cap)
        assert hip_ctx.to_host(d_out, n).tobytes() == c["H"], (name, offset)
        hip_ctx.wavelet_reset()
        hip_ctx.wavelet_routes(reset=True)
        out = np.zeros(cap, np.uint8)
        n = hip_ctx.wavelet_encode_device(d_in + offset, block.size, LF, c["freqs"], out, threads=4)
        assert out[:n].tobytes() == c["B"], (name, offset)
        _assert_device_models(hip_ctx.wavelet_routes(), blocks=1)
    finally:
        hip_ctx.dfree(d_out)
        hip_ctx.dfree(d_in)


@pytest.mark.parametrize("coder", ["b", "u"])
def test_limit_other_model_letters(coder, hip_ctx, oracle, limits):
    """The cases of at most 16 MiB with the 'b' and 'u' main models: same streams, other models."""
    try:
        for name in blockgen.LIMIT_CASE_NAMES:
            c = limits[name]
            if c["block"].size > (16 << 20):
                continue
            hip_ctx.wavelet_start(coder)
            got = hip_ctx.wavelet_encode(c["block"], LF, c["freqs"], threads=4)
            want = oracle.oracle_wavelet_encode_block_with(coder, c["block"], LF, c["freqs"])
            assert got.tobytes() == want.tobytes(), (coder, name)
    finally:
        hip_ctx.wavelet_reset()
