"""The test-side 'H' record writer (tests/hrecord.py) on the CPU: it is byte-identical to the oracle's
encoder wherever both can write the record, every hand-built case reaches the edge it is named for,
the oracle's serial decoder decodes the cases to their expected bytes and refuses the damaged records
whose damage it checks.  tests/test_gpu_huffman_decode_limits.py holds the GPU decoder to these."""
import numpy as np
import pytest

import blockgen
import hrecord
from bwtc_amd import synth
from test_coder_limits import frame

ORACLE_MAX_RUNS = 1 << 20          # larger cases are checked by construction only


def oracle_split(bwt, lf):
    """(oracle record, the same record's sections for write_record) of a transformed block."""
    import oracle_lib
    bwt = np.ascontiguousarray(bwt, np.uint8)
    freqs = np.bincount(bwt, minlength=256).astype(np.uint32)
    rec = oracle_lib.oracle_huffman_encode_block(bwt, np.asarray(lf, np.uint32), freqs)
    runs = blockgen.section_runs(bwt, oracle_lib.oracle_sections(freqs))
    return rec, [(s, l, None) for s, l in runs]


def _oracle_decodes(oracle, rec, facts):
    total = facts["total"]
    back = oracle.oracle_decode_transformed("H", frame(b"H", rec.tobytes(), total), total + 8)
    assert back is not None and back.size == total
    assert (back == hrecord.expected(facts)).all()


@pytest.mark.parametrize("name", blockgen.LIMIT_CASE_NAMES)
def test_writer_equals_oracle_on_limit_blocks(name, oracle):
    [(_, block, _)] = list(blockgen.limit_blocks(names=(name,)))
    want, secs = oracle_split(block, [0])
    got, facts = hrecord.write_record([0], secs)
    assert got.size == want.size and got.tobytes() == want.tobytes(), name
    assert facts["total"] == block.size and facts["bytes"] == want.size


def _ordinary_blocks():
    rng = np.random.default_rng(8)
    yield "text", synth.gen_text(400000, 3), 8
    yield "random", rng.integers(0, 256, 300000).astype(np.uint8), 8
    yield "all_equal", np.full(50000, 200, np.uint8), 8
    yield "n_lf_1", synth.gen_text(20000, 5), 1
    yield "n_lf_256", rng.integers(0, 256, 500000).astype(np.uint8), 256
    yield "256_sections", rng.permutation(np.arange(256 * 10000) % 256).astype(np.uint8), 8


@pytest.mark.parametrize("name", [b[0] for b in _ordinary_blocks()])
def test_writer_equals_oracle_on_ordinary_blocks(name, oracle):
    [(_, data, sp)] = [b for b in _ordinary_blocks() if b[0] == name]
    bwt, lf, _ = oracle.oracle_bwt_block(data, sp)
    want, secs = oracle_split(bwt, lf)
    if name == "n_lf_256":
        assert lf.size == 256
    if name == "256_sections":
        assert len(secs) == 256 and want[6 + (8 + 31 * lf.size + 7) // 8] == 0     # the count byte says 256
    got, facts = hrecord.write_record(lf, secs)
    assert got.tobytes() == want.tobytes(), name
    assert (hrecord.expected(facts) == bwt).all()


def test_writer_refuses_codes_that_are_not_prefix_free():
    clen = np.zeros(256, np.int64)
    clen[[1, 2]] = [1, 3]                 # canonical: 000 and 0 -- "0" is a prefix of "000"
    with pytest.raises(ValueError):
        hrecord.write_record([0], [(np.array([1, 2], np.uint8), np.ones(2), clen)])
    clen[[1, 2, 3]] = 1                   # over-full: three 1-bit codes
    with pytest.raises(ValueError):
        hrecord.write_record([0], [(np.array([1, 2, 3], np.uint8), np.ones(3), clen)])
    clen[:] = 0
    clen[[7, 9, 200]] = 2                 # incomplete but prefix-free: 00 01 10
    hrecord.write_record([0], [(np.array([7, 9, 200], np.uint8), np.ones(3), clen)])


def test_expected_chunks_join_up():
    rng = np.random.default_rng(2)
    s = rng.integers(0, 256, 500).astype(np.uint8)
    ln = rng.integers(1, 900, 500)
    _, facts = hrecord.write_record([0], [(s, ln, None), (s[:10], ln[:10], None)])
    whole = hrecord.expected(facts)
    for lo, hi in ((0, 1), (0, 7), (5, 4000), (123, facts["total"]), (facts["total"] - 1, facts["total"])):
        assert (hrecord.expected(facts, lo, hi) == whole[lo:hi]).all(), (lo, hi)


@pytest.mark.parametrize("max_len", hrecord.CODE_SHAPE_MAX_LENS)
def test_code_shape_cases(max_len, oracle):
    rec, facts = hrecord.code_shape_case(max_len)
    [sec] = facts["sections"]
    assert sec["h_M"] == max_len
    clen = hrecord.complete_code(max_len)
    assert hrecord.kraft(clen) == 1 << 64                                  # complete
    if max_len == 64:
        assert np.count_nonzero(clen) == 65 and sorted(clen[clen > 0]) == list(range(1, 64)) + [64, 64]
    assert np.isin(np.flatnonzero(clen), facts["blocks"][0][0]).all()      # every symbol used
    _oracle_decodes(oracle, rec, facts)


def test_incomplete_code_case(oracle):
    rec, facts = hrecord.incomplete_case()
    assert facts["sections"][0]["h_M"] == 2
    _oracle_decodes(oracle, rec, facts)


def test_retry_case(oracle):
    rec, facts = hrecord.retry_case()
    s = facts["sections"]
    # the deep section's stream is many times what a code fitted to its lengths gives its runs
    # (sum of len * 2^-len over the code, about 2 bits a run here): the estimate cannot hold it
    assert s[1]["h_M"] == 64 and s[1]["h_bits"] > 16 * s[1]["n_runs"]
    assert s[0]["h_bits"] == 8 * s[0]["n_runs"] and s[2]["h_bits"] == 8 * s[2]["n_runs"]
    _oracle_decodes(oracle, rec, facts)


@pytest.mark.parametrize("name,n_runs,tiles", hrecord.huffman_tile_runs())
def test_huffman_tile_cases(name, n_runs, tiles, oracle):
    rec, facts = hrecord.huffman_tiles_case(n_runs)
    [sec] = facts["sections"]
    assert sec["h_bits"] == 8 * n_runs and sec["h_tiles"] == tiles, (name, sec)
    if name.endswith("_short"):
        assert sec["h_bits"] == tiles * hrecord.TILE_BITS - 8
    if name.endswith("_past"):
        assert sec["h_bits"] == (tiles - 1) * hrecord.TILE_BITS + 8
    if n_runs <= ORACLE_MAX_RUNS:
        _oracle_decodes(oracle, rec, facts)


@pytest.mark.parametrize("name,n_runs,width,tiles", hrecord.gamma_tile_runs())
def test_gamma_tile_cases(name, n_runs, width, tiles, oracle):
    rec, facts = hrecord.gamma_tiles_case(n_runs, width)
    [sec] = facts["sections"]
    assert sec["g_bits"] == width * n_runs and sec["g_tiles"] == tiles, (name, sec)
    assert sec["g_longest"] == width
    if n_runs <= ORACLE_MAX_RUNS:
        _oracle_decodes(oracle, rec, facts)


@pytest.mark.parametrize("name", [c[0] for c in hrecord.sections_cases()])
def test_sections_cases(name, oracle):
    [(_, (rec, facts))] = [c for c in hrecord.sections_cases() if c[0] == name]
    secs = facts["sections"]
    if name == "256_sections_with_empties":
        assert len(secs) == 256 and rec[6 + 5] == 0 and sum(s["S"] == 0 for s in secs) == 85
    if name == "one_byte_sections":
        assert all(s["S"] == 1 and s["g_M"] == 1 for s in secs)
    if name == "borders_inside_runs":
        b = facts["blocks"]
        assert all(b[i][0][-1] == b[i + 1][0][0] for i in range(len(b) - 1))
    if name == "256_then_1_then_2_symbols":
        assert [np.unique(s).size for s, _ in facts["blocks"]] == [256, 1, 2]
    if name == "n_lf_256":
        assert len(facts["lf"]) == 256 and max(facts["lf"]) == (1 << 31) - 1
    _oracle_decodes(oracle, rec, facts)


def test_ceiling_cases_reach_the_32_bit_edge():
    rec, facts = hrecord.ceiling_case(hrecord.MAX_TOTAL)
    [sec] = facts["sections"]
    assert facts["total"] == 0xFFFFFFF0
    assert sec["g_longest"] == 63 and sec["g_M"] == 63                     # a run of 2^31 bytes and more
    assert int(facts["blocks"][0][1].max()) >= 1 << 31
    rec, facts = hrecord.ceiling_case(hrecord.MAX_TOTAL + 1)
    assert facts["total"] == 0xFFFFFFF1


def test_damaged_cases_are_refused_by_the_oracle_where_it_checks(oracle):
    cases = hrecord.damaged_cases()
    assert len({c[0] for c in cases}) == len(cases)
    assert {c[1] for c in cases} == {"E_SHAPE", "E_NO_CODE", "E_RUNS", "E_LENGTH", "E_PAST_RECORD"}
    for name, _, rec, checks in cases:
        if checks:
            assert oracle.oracle_decode_transformed("H", frame(b"H", rec.tobytes(), 1 << 16), 1 << 20) is None, name
