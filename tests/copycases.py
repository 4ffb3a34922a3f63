"""The blocks of the copy rounds' tests (tests/test_gpu_copy_rounds.py), built here so that tests/test_copymodel.py can
prove, without a GPU, that every named block has the edge it is named for: the rounds tests/copymodel.py takes with the
rule and without it.

The blocks are written as the sorter's T; block() turns one into what a caller hands to bwt_block(), which sorts the
reverse.  Copies of a piece reversed are copies of the reversed piece."""
import numpy as np

import periodcases as pc

LETTERS = np.arange(97, 123, dtype=np.uint8)
WORDS = [b"the", b"of", b"and", b"copy", b"round", b"suffix", b"sorter", b"rank", b"depth", b"list", b"group", b"tied", b"piece", b"a"]


def block(T):
    """What bwt_block() is handed for the sorter to see T."""
    return np.ascontiguousarray(np.asarray(T, np.uint8)[::-1])


def letters(n, seed):
    """n random lower-case letters: no repeats to speak of."""
    return LETTERS[np.random.default_rng([61, n, seed]).integers(0, 26, n)]


def words(n, seed):
    """n bytes of words from a short list: a piece with inner repeats."""
    rng = np.random.default_rng([67, n, seed])
    out, have = [], 0
    while have < n:
        w = WORDS[int(rng.integers(0, len(WORDS)))] + b" "
        out.append(np.frombuffer(w, np.uint8))
        have += len(w)
    return np.concatenate(out)[:n].copy()


def copies(piece, count, seed=0, lo=1, hi=300):
    """`count` copies of `piece`, each behind a filler of lo ... hi bytes of its own (symbols no piece holds)."""
    rng = np.random.default_rng([71, count, seed])
    parts = []
    for i in range(count):
        parts += [pc.filler(int(rng.integers(lo, hi + 1)), 1000 * seed + i), piece]
    parts.append(pc.filler(7, 1000 * seed + count))
    return pc.cat(*parts)


def shuffled(pieces, each, seed=0):
    """`each` copies of every piece in a random order, nothing between them."""
    rng = np.random.default_rng([73, len(pieces), each, seed])
    which = np.repeat(np.arange(len(pieces)), each)
    rng.shuffle(which)
    return pc.cat(*[pieces[i] for i in which], pc.filler(5, seed))


# (name, T, what the premise is: the model with the rule takes at most `with_` rounds from depth 16, the plain one at least `plain`)
def copy_blocks():
    return [
        ("2 copies of 64 KiB of letters", copies(letters(1 << 16, 1), 2, 1), 2, 11),
        ("12 copies of 16 KiB of letters", copies(letters(1 << 14, 2), 12, 2), 2, 9),
        ("300 copies of 1 KiB of letters", copies(letters(1 << 10, 3), 300, 3), 2, 5),
        ("12 copies of 16 KiB of words", copies(words(1 << 14, 4), 12, 4), 3, 9),
        ("two pieces, 6 + 6 copies shuffled", shuffled([letters(1 << 14, 5), letters(1 << 14, 6)], 6, 5), 4, 9),
    ]


def plain_blocks():
    """(name, T): blocks without copies -- the rule may change neither rounds nor route."""
    rng = np.random.default_rng(79)
    return [
        ("random bytes", rng.integers(0, 256, 200000).astype(np.uint8)),
        ("random letters", letters(150000, 7)),
        ("four symbols", rng.integers(0, 4, 100000).astype(np.uint8)),
    ]


def step_blocks():
    """(name, T, route bit): copies beside a long run (bit 5) or a long stretch of period 9 (bit 8) -- the closed-form step
    runs, and a block with a step takes no copy round."""
    twelve = copies(letters(1 << 14, 8), 12, 8)
    return [
        ("copies and a run", pc.cat(twelve, np.zeros(1 << 16, np.uint8), pc.filler(300, 81)), 32),
        ("copies and a stretch of period 9", pc.cat(twelve, pc.stretch(9, 1 << 16), pc.filler(300, 82)), 256),
    ]


def random_block(it):
    """Block `it` of the randomised case, at most 64 KiB -> (T, starting points): 2 ... 40 copies of one or two pieces of
    letters or words, behind fillers or shuffled, a tail of noise."""
    rng = np.random.default_rng([20260303, it])
    kinds = int(rng.integers(1, 3))
    count = int(rng.integers(2, 41))
    size = max(64, int(rng.integers(1 << 10, 1 << 14)) // count)
    make = words if it % 3 == 0 else letters
    pieces = [make(size + 13 * j, 100 * it + j) for j in range(kinds)]
    if it % 4 == 1 and kinds == 2:
        T = shuffled(pieces, max(2, count // 2), it)
    else:
        T = pc.cat(*[copies(q, count, it + j, 1, int(rng.integers(1, 300))) for j, q in enumerate(pieces)])
    T = pc.cat(T, pc.filler(int(rng.integers(0, 2000)), 300 + it))
    assert T.size <= 1 << 16
    return T, (1, 8)[it % 2]
