"""tests/copymodel.py (the rule for whole copies, BWTC_HIP_COPIES=1) held to sorted() and to tests/runmodel.py's plain
sorter, and the premises of tests/copycases.py's blocks.  No GPU."""
import itertools

import numpy as np
import pytest

import copycases as cases
import copymodel as cm
import runmodel

DEPTHS = (1, 2, 3)


def _truth(T):
    return sorted(range(len(T)), key=lambda s: T[s:])


def _texts(sigma, longest):
    """Every string of 1 ... longest letters over sigma symbols, each behind the terminator."""
    for n in range(1, longest + 1):
        for t in itertools.product(range(1, sigma + 1), repeat=n):
            yield bytes(t) + b"\0"


@pytest.mark.parametrize("sigma,longest", [(2, 12), (3, 8)])
def test_exhaustive(sigma, longest):
    """Every string up to 12 over 2 letters and up to 8 over 3, at depths 1, 2, 3: the order is sorted()'s, with the
    model's assertions on (one K per group, K + h characters shared), with the gate and without."""
    count = 0
    for T in _texts(sigma, longest):
        want = _truth(T)
        for depth in DEPTHS:
            order, rounds, passes = cm.sort_suffixes(T, depth)
            assert order == want, (T, depth)
            assert passes <= rounds
            count += 1
        assert cm.sort_suffixes(T, 1, gate=False)[0] == want, T
    assert count == 3 * sum(sigma ** n for n in range(1, longest + 1))


def _piece_and_filler(seed):
    """A short text of copies of one or two pieces over a few letters behind fillers of 0 ... 3 bytes."""
    rng = np.random.default_rng([83, seed])
    sigma = int(rng.integers(2, 5))
    pieces = [rng.integers(1, sigma + 1, int(rng.integers(2, 14))).astype(np.uint8) for _ in range(int(rng.integers(1, 3)))]
    parts = []
    for _ in range(int(rng.integers(2, 7))):
        parts += [rng.integers(1, sigma + 2, int(rng.integers(0, 4))).astype(np.uint8), pieces[int(rng.integers(0, len(pieces)))]]
    parts.append(rng.integers(1, sigma + 1, int(rng.integers(0, 3))).astype(np.uint8))
    return bytes(np.concatenate(parts)) + (b"\0" if seed % 2 else b"")


def test_random_pieces_and_fillers():
    for seed in range(3000):
        T = _piece_and_filler(seed)
        want = _truth(T)
        for depth in DEPTHS:
            assert cm.sort_suffixes(T, depth)[0] == want, (T, depth)


def test_without_the_rule_it_is_the_plain_sorter():
    for seed in range(400):
        T = _piece_and_filler(seed)
        for depth in DEPTHS:
            order, rounds, passes = cm.sort_suffixes(T, depth, copies=False)
            plain, plain_rounds, _ = runmodel.sort_suffixes(T, depth, runs=False)
            assert (order, rounds, passes) == (plain, plain_rounds, 0), (T, depth)


def test_the_twins_agree():
    """sort_suffixes_np() and copy_lengths_np() against the lists' forms."""
    for seed in range(300):
        T = _piece_and_filler(seed)
        for depth in DEPTHS:
            for gate in (True, False):
                order, rounds, passes = cm.sort_suffixes(T, depth, gate=gate)
                order_np, rounds_np, passes_np, _ = cm.sort_suffixes_np(np.frombuffer(T, np.uint8), depth, gate=gate)
                assert (order, rounds, passes) == (order_np.tolist(), rounds_np, passes_np), (T, depth, gate)


@pytest.mark.parametrize("name,T", [("zeros", np.zeros(5000, np.uint8)), ("period 9", np.tile(np.arange(1, 10, dtype=np.uint8), 600)),
                                    ("random letters", cases.letters(20000, 0)), ("16 copies back to back", np.tile(cases.letters(512, 1), 16))])
def test_no_more_rounds_where_the_rule_does_not_apply(name, T):
    """Zeros, period 9, random letters and back-to-back copies (a period: not covered) take equal rounds with the rule and
    without, from depths 1 and 16."""
    for depth in (1, 16):
        order, with_, _, _ = cm.sort_suffixes_np(T, depth)
        plain_order, plain, _, _ = cm.sort_suffixes_np(T, depth, copies=False)
        assert (order == plain_order).all() and with_ <= plain, (name, depth, with_, plain)
        if name != "random letters":
            assert with_ == plain, (name, depth, with_, plain)


@pytest.mark.parametrize("which", range(5))
def test_premises_of_the_copy_blocks(which):
    """Every block of copycases.copy_blocks(), as the sorter sees it and reversed, from depths 16 and 48: the rule takes at
    most `with_` rounds, the plain sorter at least `plain`, and the orders agree."""
    name, T, most, least = cases.copy_blocks()[which]
    for X in (T, cases.block(T)):
        for depth in (16, 48):
            order, with_, passes, entries = cm.sort_suffixes_np(X, depth)
            plain_order, plain, _, plain_entries = cm.sort_suffixes_np(X, depth, copies=False)
            print("%s from %d: %d rounds (%d passes, %d entries) against %d (%d entries)" % (name, depth, with_, passes, entries, plain, plain_entries))
            assert (order == plain_order).all(), (name, depth)
            assert with_ <= most and plain >= least - (2 if depth == 48 else 0) and passes <= with_, (name, depth, with_, plain, passes)


def test_premises_of_the_other_blocks():
    """The plain blocks take equal rounds with the rule and without; the step blocks hold the run or the stretch they name."""
    for name, T in cases.plain_blocks():
        with_, plain = cm.sort_suffixes_np(T, 4)[1], cm.sort_suffixes_np(T, 4, copies=False)[1]
        assert with_ == plain, (name, with_, plain)
    import periodmodel
    for name, T, bit in cases.step_blocks():
        p = 1 if bit == 32 else 9
        assert periodmodel.period_lengths_np(T, p)[1] >= 1 << 16, name
    for it in range(100):
        T, sp = cases.random_block(it)
        assert T.size <= 1 << 16 and sp in (1, 8)
