"""The suffix sorter's code-key stage on the GPU (-m gpu), kernel by kernel: k_pair_counts, k_code_build and
k_make_keys_code of bwtc_amd/csrc/bwt_engine.hip through the hooks bwtc_hip_test_code_stage / _table / _keys, with the
launch shapes and the key layout of BwtEngine::suffix_sort, held to tests/codemodel.py by exact equality: dense codes,
pair counts, every table entry, the error word, and every suffix's key word, second word and plane byte.  The named
cases and their inputs are codemodel.cases() / make(); tests/test_codemodel.py shows the model's tables prefix free,
alphabetic, complete and short, its keys monotone with honest levels, and every case at the edge it is named for.  The
hooks check their contracts on the host and guard the keys, the second words, the plane and the table with canaries (a
changed one raises)."""
import numpy as np
import pytest

import codemodel as cm
from bwtc_amd import hip

pytestmark = pytest.mark.gpu


def _same(name, what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or not np.array_equal(got, want):
        bad = np.flatnonzero(got.ravel() != want.ravel()) if got.shape == want.shape else []
        first = int(bad[0]) if len(bad) else -1
        raise AssertionError("%s: %s differs at %d of %d places, first at %d: got %s, want %s" % (
            name, what, len(bad), want.size, first, hex(int(got.ravel()[first])) if first >= 0 else got.shape,
            hex(int(want.ravel()[first])) if first >= 0 else want.shape))


def _same_keys(c, keys, w, plane, want):
    _same(c["name"], "w", w, want["w"])
    _same(c["name"], "keys", keys, want["keys"])
    _same(c["name"], "plane", plane, want["plane"])


def _run_stage(ctx, c):
    inp = cm.make(c)
    want = cm.expected(c, inp)
    got = ctx.test_code_stage(inp["T"], c["lone"], c["kbits"], c["split"], want_keys=c["want_keys"])
    _same(c["name"], "lut", got["lut"], want["lut"])
    assert got["sigma"] == want["sigma"], c["name"]
    _same(c["name"], "counts", got["counts"], want["counts"])
    _same(c["name"], "table", got["table"], want["table"])
    assert got["err"] == want["err"] == 0, c["name"]
    if c["want_keys"]:
        _same_keys(c, got["keys"], got["w"], got["plane"], want)
    return inp, want, got


@pytest.mark.parametrize("bucket", cm.buckets("counts"))
def test_pair_counts_at_the_seams(hip_ctx, bucket):
    """The whole stage over n in {1, 2, 15, 16, 17, 4095, 4096, 4097, 8 * 4096 + 5}, 511 * 4096 + 3 and 512 * 4096 (every
    tile sampled once, the first ending in a partial tile), 513 * 4096 + 7 and 1500 * 4096 + 1 (the sample skips tiles; 6 MiB,
    the only case of that size: the sample's stride only passes 2 at 1024 tiles, so nothing smaller takes tiles 0, 2, 5, ...).
    The texts carry a pair that occurs nowhere else across the 16-byte thread seams, the 4096 tile seams, at position 0 and
    at position n - 1; with a zero byte among the symbols and with the lone terminator, whose merged code 0 counts with the
    smallest symbol.  Counts summed over the replicas, the table and -- up to 70 000 suffixes -- the keys."""
    cs = [c for c in cm.cases("counts") if c["bucket"] == bucket]
    assert cs
    for c in cs:
        _run_stage(hip_ctx, c)


@pytest.mark.parametrize("bucket", cm.buckets("table"))
def test_code_table_from_given_counts(hip_ctx, bucket):
    """k_code_build alone, sigma in {1, 2, 3, 4, 255, 256}: all counts zero (the balanced tree), one count of 2^21 among
    zeros, row totals of 65535 and 65536 (the shift goes from 0 to 1), equal weights (a tie at every cut, sigma odd and
    even), doubling, Fibonacci and tripling weights ascending and descending (the deepest trees: 17 bits at sigma 255
    and 256, the deepest codeword seen in any case; 26 is the limit), all the weight at the last symbol and at the first.
    Equal to the model entry by entry, error word 0, and the device's own table prefix free, alphabetic and complete."""
    cs = [c for c in cm.cases("table") if c["bucket"] == bucket]
    assert cs
    for c in cs:
        inp = cm.make(c)
        want = cm.expected(c, inp)
        table, err = hip_ctx.test_code_table(inp["counts"], c["sigma"])
        _same(c["name"], "table", table, want["table"])
        assert err == want["err"] == 0, c["name"]
        chk = cm.table_checks(table, c["sigma"])
        assert chk["ok"] and chk["prefix_free"] and chk["alphabetic"] and chk["complete"], (c["name"], chk)
        assert chk["longest"] <= cm.MAX_LEN, (c["name"], chk["longest"])
        if c["kind"] == "zeros":
            lens = table[:, :c["sigma"]] >> 27
            assert max(1, c["sigma"].bit_length() - 1) <= int(lens.min()) and int(lens.max()) <= max(1, (c["sigma"] - 1).bit_length())


@pytest.mark.parametrize("bucket", cm.buckets("keys"))
def test_key_maker_with_given_tables(hip_ctx, bucket):
    """k_make_keys_code alone.  sizes-*: n in {1, 2, 3, 1023, 1024, 1025, 2049, 65536 + 1025} (the last split with non-zero
    upper bits, and unsplit) times kbits in {40, 41, 63, 64, 65, 71, 72}, random text, with every context codeword one bit
    (sigma 2: 71 codewords behind the first, the whole 72-character look-ahead, level 7), every codeword 26 bits (sigma 256:
    the tile's bit string at its fullest, level 0) and a comb of 1-bit and 26-bit codewords (they straddle the 32-bit
    words at every offset).  texts-*: one symbol repeated, a tail of 80 other symbols (the padding's codewords in the
    last keys), the terminator under lone_sentinel.  levels: fixed lengths l0 and L with 1 + (kbits - l0) / L in
    {7, 8, 11, 12, 15, 16, 19, 20, 23, 24, 31, 32, 47, 48}.  need: l0 in 9..26 at kbits 40 (need 14..31), l0 = 8 at 40 and
    72 (need 32 and 64), l0 in 1..7 at 72 (need 65..71)."""
    cs = [c for c in cm.cases("keys") if c["bucket"] == bucket]
    assert cs
    for c in cs:
        inp = cm.make(c)
        want = cm.expected(c, inp)
        keys, w, plane = hip_ctx.test_code_keys(inp["T"], inp["lut"], inp["sigma"], inp["table"], c["kbits"], c["split"])
        _same_keys(c, keys, w, plane, want)


@pytest.mark.parametrize("bucket", cm.buckets("stage"))
def test_whole_stage_on_structured_text(hip_ctx, bucket):
    """The whole stage with the product's own table on structured text (words, planted repeats, a periodic stretch, a
    run) of 5 003 to 60 000 bytes over 2, 20, 60 and 230 symbols, with zero bytes and with the lone terminator, code_bits
    40, 48 and 72: every output equal to the chained model, and the device's keys held to the two properties the
    ranking and the finisher rely on, against sorted() over the dense-code strings: monotone, and honest levels."""
    cs = [c for c in cm.cases("stage") if c["bucket"] == bucket]
    assert cs
    for c in cs:
        inp, want, got = _run_stage(hip_ctx, c)
        hi, lo, level = cm.unpack(got["keys"], got["w"], c["kbits"], c["split"])
        order = cm.suffix_order(inp["T"], got["lut"])
        assert cm.monotone_breaks(order, hi, lo) == 0, c["name"]
        assert cm.level_breaks(order, hi, lo, level, inp["T"], got["lut"]) == 0, c["name"]


def _refused(call):
    with pytest.raises(hip.BwtcHipError) as e:
        call()
    return e.value.code


def test_contract_refusals(hip_ctx):
    """Host checks of the hooks: nothing malformed is launched (-1), and the context still makes keys afterwards."""
    c = [c for c in cm.cases("keys") if c["bucket"] == "need"][0]
    inp = cm.make(c)
    T, lut, sigma, table = inp["T"], inp["lut"], inp["sigma"], inp["table"]
    ctx = hip_ctx
    assert _refused(lambda: ctx.test_code_keys(T[:0], lut, sigma, table)) == -1                           # n = 0
    assert _refused(lambda: ctx.test_code_keys(T, lut, sigma, table, code_bits=39)) == -1
    assert _refused(lambda: ctx.test_code_keys(T, lut, sigma, table, code_bits=73)) == -1
    assert _refused(lambda: ctx.test_code_keys(T, lut, 0, table)) == -1
    assert _refused(lambda: ctx.test_code_keys(T, lut, 257, table)) == -1
    assert _refused(lambda: ctx.test_code_keys(np.zeros((64 << 20) + 1024, np.uint8), lut, sigma, table)) == -1   # no room for the canaries
    wrong = lut.copy()
    wrong[int(T[5])] = sigma                                                                              # a byte of T without a codeword
    assert _refused(lambda: ctx.test_code_keys(T, wrong, sigma, table)) == -1
    wrong = lut.copy()
    wrong[0] = sigma                                                                                      # the padding's byte
    assert _refused(lambda: ctx.test_code_keys(T[T > 0], wrong, sigma, table)) == -1
    for row, entry in ((3, (27 << 27) | 1), (256, 0), (0, (3 << 27) | 8), (255, table[255, 0])):             # too long, no length, bits above the length, a codeword twice
        bad = table.copy()
        bad[row, 1] = entry
        assert _refused(lambda: ctx.test_code_keys(T, lut, sigma, bad)) == -1
    bad = table.copy()
    bad[7, 2] = (2 << 27) | int((table[7, 3] & 0x7FFFFFF) >> ((table[7, 3] >> 27) - 2))                   # a prefix of its neighbour
    assert _refused(lambda: ctx.test_code_keys(T, lut, sigma, bad)) == -1
    counts = np.zeros((256, 256), np.uint32)
    counts[0, 0], counts[9, 9] = 1 << 21, 1
    assert _refused(lambda: ctx.test_code_table(counts, 4)) == -1                                          # more pairs than a sample has
    counts[9, 9] = 0
    assert _refused(lambda: ctx.test_code_table(counts, 0)) == -1
    assert _refused(lambda: ctx.test_code_table(counts, 257)) == -1
    S = np.array([5, 6, 0, 7, 0], np.uint8)
    assert _refused(lambda: ctx.test_code_stage(S, True)) == -1                                            # a zero byte besides the terminator
    assert _refused(lambda: ctx.test_code_stage(S[:4], True)) == -1                                        # no terminator
    assert _refused(lambda: ctx.test_code_stage(S[:0], False)) == -1
    assert _refused(lambda: ctx.test_code_stage(S, False, code_bits=39)) == -1
    # and the context still works
    keys, w, plane = ctx.test_code_keys(T, lut, sigma, table, c["kbits"], c["split"])
    _same_keys(c, keys, w, plane, cm.expected(c, inp))
    table4, err = ctx.test_code_table(counts, 4)
    assert err == 0 and np.array_equal(table4, cm.build_table(counts, 4)[0])
    got = ctx.test_code_stage(S, False)
    assert got["sigma"] == 4 and got["err"] == 0 and int(got["counts"].sum()) == 4
