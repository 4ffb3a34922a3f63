"""The batched sorter's rule (tests/batchmodel.py) against sorted() and the oracle; no GPU."""
import itertools

import numpy as np
import pytest

import batchcases
import batchmodel


def _want_order(blocks, k):
    """positions by (block, suffix as a byte string): Python compares bytes lexicographically, a proper prefix first"""
    texts = batchmodel._texts(blocks)
    items = [((b, t[i:]), (b << k) + i) for b, t in enumerate(texts) for i in range(len(t))]
    return [s for _, s in sorted(items)]


TWO_LETTER_BLOCKS = [bytes(t) for n in range(1, 6) for t in itertools.product((0, 1), repeat=n)]


def test_scalar_rule_is_sorted_exhaustively():
    """All batches of one to three blocks of length 1 ... 5 over {0, 1}, the rule's assertions on."""
    assert len(TWO_LETTER_BLOCKS) == 62
    count = 0
    for k in (1, 2, 3):
        for blocks in itertools.product(TWO_LETTER_BLOCKS, repeat=k):
            res = batchmodel.sort_scalar(blocks)
            assert res["order"] == _want_order(blocks, res["k"]), blocks
            count += 1
    assert count == 62 + 62 ** 2 + 62 ** 3


@pytest.mark.parametrize("key_chars", [1, 2])
def test_scalar_rule_rounds_exhaustively(key_chars):
    """Six characters settle every suffix of a five-byte block: the same batches (one and two blocks) under keys of one
    and two characters go through rounds at depths 1, 2, 4 / 2, 4, where suffixes do end at and below the depth."""
    deepest = 0
    for k in (1, 2):
        for blocks in itertools.product(TWO_LETTER_BLOCKS, repeat=k):
            res = batchmodel.sort_scalar(blocks, key_chars)
            assert res["order"] == _want_order(blocks, res["k"]), blocks
            deepest = max(deepest, res["rounds"])
    assert deepest == (3 if key_chars == 1 else 2)


def test_numpy_rule_equals_scalar_rule():
    rng = np.random.default_rng(3)
    batches = [batchcases.random_batch(rng)[0] for _ in range(40)]
    batches += [list(b) for b in itertools.islice(itertools.product(TWO_LETTER_BLOCKS, repeat=3), 0, None, 997)]
    for blocks in batches:
        blocks = [b for b in blocks][:20]
        for key_chars in (1, 6):
            want = batchmodel.sort_scalar([bytes(bytearray(b)) for b in blocks], key_chars)
            bt = batchmodel.Batch(blocks)
            rank, rounds, active = batchmodel.sort_batch(bt, key_chars, check=True)
            assert rounds == want["rounds"] and active == want["active"]
            assert [want["rank"][int(s)] for s in bt.positions()] == rank.tolist()


@pytest.mark.parametrize("name", sorted(batchcases.CASES))
def test_case_premise_and_oracle(name):
    batchcases.premise(name)
    res = batchcases.model(name)
    want = batchcases.oracle(name)
    assert len(res["blocks"]) == len(want)
    for b, (got, ora) in enumerate(zip(res["blocks"], want)):
        for part, g, w in zip(("bytes", "lf", "freqs"), got, ora):
            assert g.shape == w.shape and (g == w).all(), (name, b, part)


def test_keys_have_the_stated_fields():
    blocks = [b"\0", b"\0\0ab", bytes(range(1, 10))]
    T, keys, counts = batchmodel.keys_and_text(blocks)
    assert T.tobytes() == b"\0\0" + b"ba\0\0\0" + bytes(range(9, 0, -1)) + b"\0"
    k = [int(v) for v in keys]
    assert [v >> 51 for v in k] == [0, 0] + [1] * 5 + [2] * 10
    assert [v & 7 for v in k] == [2, 1, 5, 4, 3, 2, 1, 6, 6, 6, 6, 6, 5, 4, 3, 2, 1]
    assert (k[7] >> 3) & ((1 << 48) - 1) == int.from_bytes(bytes([9, 8, 7, 6, 5, 4]), "big")
    assert (k[2] >> 3) & ((1 << 48) - 1) == int.from_bytes(b"ba\0\0\0\0", "big")
    assert len(set(k)) == len(k)                            # the zero suffixes of block 1 differ by their length field alone
    assert counts[1][0] == 2 and counts[1][0x61] == 1 and counts.sum() == 14
