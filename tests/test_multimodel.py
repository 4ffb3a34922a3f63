"""tests/multimodel.py held to sorted(), to tests/mixedmodel.py and to its numpy twin, what the merge buys, the finder's
candidates and the host's rule, and the premises of the blocks in tests/multicases.py (no GPU, no library)."""
import itertools

import numpy as np
import pytest

import mixedcases as mc
import mixedmodel
import multicases as cases
import multimodel as mu
import periodcases as pc
import periodmodel
from periodmodel import PERIOD_MAX

SUBSETS = [c for r in (1, 2, 3, 4) for c in itertools.combinations((1, 2, 3, 4), r)]
DEPTHS = (1, 2, 3, 4)


def _sorted(T):
    T = bytes(T)
    return sorted(range(len(T)), key=lambda s: T[s:])


def _exhaustive(letters, length):
    steps = several = 0
    for tup in itertools.product(letters, repeat=length):
        T = bytes(tup)
        want = _sorted(T)
        lengths = {p: (periodmodel.period_lengths(T, p)[0], mu.gate_length(T, p)) for p in (1, 2, 3, 4)}
        for periods in SUBSETS:
            for depth in DEPTHS:
                order, rounds, ran = mu.sort_suffixes(T, periods, depth, check=True, lengths=lengths)
                assert order == want, (T, periods, depth)
                assert all(at >= p and p in periods for p, at in ran) and len({p for p, _ in ran}) == len(ran), (T, periods, depth, ran)
                steps += bool(ran)
                several += len(ran) > 1
    return steps, several


@pytest.mark.parametrize("length", range(1, 13))
def test_every_string_over_two_letters(length):
    """Every string over 2 letters of this length, every non-empty subset of the periods 1 ... 4, depths 1 ... 4, with the
    model's own assertions on: sorted()'s order, every step at a depth that reaches its period, no period twice."""
    steps, several = _exhaustive(b"ab", length)
    assert length < 8 or (steps > 0 and several > 0), (steps, several)


@pytest.mark.parametrize("length", range(1, 9))
def test_every_string_over_three_letters(length):
    steps, several = _exhaustive(b"abc", length)
    assert length < 8 or (steps > 0 and several > 0), (steps, several)


def test_random_structured_blocks():
    """2200 blocks of up to 400 bytes with stretches of two to four periods, runs, noise and shared tails: sorted()'s
    order from the merged and from the overwrite form; every eleventh block with the model's assertions on."""
    several = three = fewer = more = 0
    for seed in range(2200):
        T, periods = cases.model_text(seed)
        want = _sorted(T)
        depth = (1, 2, 3, 5, 8)[seed % 5]
        order, rounds, ran = mu.sort_suffixes(T, periods, depth, check=seed % 11 == 0)
        assert order == want, (seed, periods, depth)
        over, over_rounds, _ = mu.sort_suffixes(T, periods, depth, merge=False)
        assert over == want, (seed, periods, depth, "overwrite")
        several += len(ran) > 1
        three += sum(p >= 2 for p, _ in ran) == 3
        fewer += rounds < over_rounds
        more += rounds > over_rounds
    print("%d blocks took several steps, %d three period steps; the merge saved rounds in %d and cost rounds in %d" % (several, three, fewer, more))
    assert several >= 800 and three >= 20 and fewer >= 50, (several, three, fewer, more)


def test_one_period_is_the_mixed_model():
    """The run step and ONE period: the same order, rounds and steps as tests/mixedmodel.py, pure and numpy."""
    two = 0
    for seed in range(260):
        T, p = mc.model_text(seed)
        for depth in (1, 2, 3, 4, 5, 8):
            want = mixedmodel.sort_suffixes(T, p, depth)
            got = mu.sort_suffixes(T, (1, p), depth)
            assert got == want, (seed, p, depth, got[1:], want[1:])
            two += len(got[2]) == 2
        got = mu.sort_suffixes_np(np.frombuffer(T, np.uint8), (1, p), 3)
        want = mixedmodel.sort_suffixes(T, p, 3)
        assert got[0].tolist() == want[0] and got[1:] == want[1:], (seed, p)
    assert two >= 200, two


def test_the_numpy_twin():
    for seed in range(300):
        T, periods = cases.model_text(seed)
        A = np.frombuffer(T, np.uint8)
        for depth in (1, 3, 8):
            for merge in (True, False):
                order, rounds, ran = mu.sort_suffixes(T, periods, depth, merge=merge)
                got = mu.sort_suffixes_np(A, periods, depth, merge=merge)
                assert got[0].tolist() == order and got[1] == rounds and got[2] == ran, (seed, periods, depth, merge, got[1:], rounds, ran)
        for p in periods:
            assert mu.gate_length_np(A, p) == mu.gate_length(T, p)


def test_merge_words():
    """The word the merging pass stores, case by case."""
    kp = np.array([5, 5, 5, 5, 9, 2], np.uint32)
    old = np.array([0, 5, 6, 4 | mu.MEMBER, 100 | mu.MEMBER, 0], np.uint32)
    assert mu.merge_words(old, kp, 5).tolist() == [5 | mu.MEMBER, 5 | mu.MEMBER, 6, 5 | mu.MEMBER, 100, 0]
    assert mu.merge_words(old, kp, 6).tolist() == [0, 5, 6, 4, 100, 0]
    assert mu.merge_words(old, kp, 5, fresh=True).tolist() == [x | mu.MEMBER for x in (5, 5, 5, 5, 9)] + [0]


def test_what_the_merge_buys():
    """The merge case: three equal stretches per period behind equal tails.  The merged form takes fewer rounds than the
    overwrite form, and than no steps at all."""
    T = cases.merge_case()
    for depth in (4, 8, 16):
        _, merged, ran = mu.sort_suffixes_np(T, (1, 9, 12), depth)
        _, over, _ = mu.sort_suffixes_np(T, (1, 9, 12), depth, merge=False)
        _, none, _ = mu.sort_suffixes_np(T, (), depth)
        print("depth %d: merged %d rounds, overwrite %d, no steps %d; steps %s" % (depth, merged, over, none, ran))
        assert [p for p, _ in ran] == [9, 12] and merged < over and merged < none, (depth, merged, over, none, ran)


# ---- the finder's candidates and the host's rule --------------------------------------------------

def _candidates_by_hand(table, need):
    found = sorted(((int(table[d]), -d) for d in range(2, PERIOD_MAX + 1) if table[d] >= need and table[d] > 0), reverse=True)
    return [(-d, v) for v, d in found[:8]]


@pytest.mark.parametrize("need", [256, 16384])
def test_candidates(need):
    seen = {}
    for name, table in cases.vote_tables(need):
        got = mu.candidates(table, need)
        assert got == _candidates_by_hand(table, need), name
        seen[name] = got
    assert seen["no bin over need"] == [] and seen["one bin at need"] == [(777, need)]
    assert len(seen["exactly 8"]) == 8 and [d for d, _ in seen["exactly 8"]] == [4096, 2, 64, 4000, 12, 300, 9, 5]
    assert len(seen["more than 8"]) == 8 and seen["more than 8"][0][1] == need + 39
    assert [d for d, _ in seen["equal votes"]] == [2, 5, 6, 17, 18, 250, 999, 1000]
    assert [d for d, _ in seen["equal votes among different ones"]] == [100, 4, 17, 40, 3000]
    assert seen["bins 2 and 4096"] == [(4096, need + 1), (2, need)]
    assert seen["votes in bins 0 and 1"] == [(33, need)]
    assert [d for d, _ in seen["every bin at need"]] == list(range(2, 10))
    assert seen["votes of 32 bits"] == [(7, 0xFFFFFFFF), (8, 0xFFFFFFFE)]


def test_accept():
    """Candidates in vote order -> entries: multiples and divisors of an accepted period are skipped, a short stretch is not
    worth a step, a multiple above the depth is divided, and three entries are the most."""
    T = cases.stretches((9, 12), 1 << 15)
    assert [p for p, _, _ in mu.accept(T, [(9, 900), (12, 800)], 8)] == [9, 12]
    assert [p for p, _, _ in mu.accept(T, [(9, 900), (18, 850), (12, 800), (3, 700)], 8)] == [9, 12]
    assert [p for p, _, _ in mu.accept(T, [(36, 900)], 8)] in ([9], [12])             # 36 divides down to one of them
    assert [p for p, _, _ in mu.accept(T, [(27, 900), (24, 800)], 8)] == [9, 12]
    assert mu.accept(T, [(7, 900)], 8) == []
    short = cases.stretches((9, 12), 8 * 12 - 1, noise=500)
    assert [p for p, _, _ in mu.accept(short, [(12, 900), (9, 800)], 8)] == [9]          # 95 < 8 x 12, 95 >= 8 x 9
    four = cases.stretches((5, 7, 11, 13), 4000, noise=300)
    got = mu.accept(four, [(13, 900), (11, 800), (7, 700), (5, 600)], 4)
    assert [p for p, _, _ in got] == [13, 11, 7] and all(3990 <= g <= 4010 for _, g, _ in got), got
    a, b = cases.DIVISOR_PAIR
    assert [p for p, _, _ in mu.accept(cases.stretches((a, b), 1 << 15), [(b, 900), (a, 800)], 8)] == [b]
    assert [p for p, _, _ in mu.accept(cases.stretches((a, b), 1 << 15), [(a, 900), (b, 800)], 8)] == [a]


# ---- the premises of tests/multicases.py ---------------------------------------------------------

def test_premises_of_the_merge_blocks():
    """Breaks one before, on and one after the seams of a thread, a wave and a tile, wherever the block holds them; old
    words on both sides of k_p; depths on both sides of a length that occurs."""
    for p in cases.MERGE_PERIODS:
        for n in cases.MERGE_SIZES:
            for delta in (-1, 0, 1):
                T = cases.merge_text(n, p, delta)
                assert T.size == n
                kp = periodmodel.period_lengths_np(T, p)[0]
                breaks = set((np.flatnonzero(T[p:] != T[:-p]) + p).tolist()) if n > p else set()
                assert breaks == {q + delta for q in cases.MERGE_SEAMS + (n - 2,) if p <= q + delta < n}, (p, n, delta)
                depths = cases.merge_depths(kp)
                assert all(h >= 1 for h in depths) and int(kp[n // 3]) in depths + [0]
                olds = dict(cases.merge_olds(kp, delta))
                assert (olds["k_p + 1"] == kp + 1).all() and (olds["random"] >> 31).any() == (n > 4)
    big = periodmodel.period_lengths_np(cases.merge_text(5 * 16384 + 17, 9, 0), 9)[0]
    took = mu.merge_words(cases.merge_olds(big, 0)[3][1], big, cases.merge_depths(big)[1])
    assert 0 < (took >> 31).sum() < big.size


def test_premises_of_the_step_blocks():
    """Every planted stretch is the longest proper stretch of its period, in T and reversed, and is worth its step at every
    depth up to 16; the planted periods lead the vote with max(256, n / 64) votes or more."""
    for periods in cases.PAIRS + (cases.DIVISOR_PAIR,) + tuple(cases.TRIPLES):
        for L in (1 << 16, 1 << 18):
            T = cases.stretches(periods, L, run=(1 << 16) if periods == (9, 300) else 0)
            assert T.size <= 1 << 20
            for X in (T, cases.block(T)):
                _, proper = cases.facts(X, periods)
                for p in periods:
                    assert L - p <= proper[p] <= L + p and proper[p] >= mu.WORTH * max(16, p), (periods, L, p, proper)
        if periods != cases.DIVISOR_PAIR:
            table = cases.vote_table(cases.stretches(periods, 1 << 16), 8)
            found = mu.candidates(table, max(256, T.size // 64))
            assert set(periods) <= {d for d, _ in found}, (periods, found)
            assert sorted(p for p, _, _ in mu.accept(cases.stretches(periods, 1 << 16), found, 8)) == sorted(cases.TRIPLES.get(periods, periods)), (periods, found)
    T = cases.merge_case()
    _, proper = cases.facts(T, (9, 12))
    assert 20000 - 12 <= proper[9] <= 20012 + 48 and 20000 - 12 <= proper[12] <= 20012 + 48, proper
    for p, q in ((9, 12), (64, 300)):
        for name, T in cases.seam_blocks(p, q):
            _, proper = cases.facts(T, (p, q))
            assert proper[p] >= 30000 - p and proper[q] >= 30000 - q, (p, q, name, proper)
        blocks = dict(cases.seam_blocks(p, q))
        T = blocks["a stretch reaches the end"]
        assert periodmodel.period_lengths_np(T, q)[0][T.size - 30000] == 30000
        assert periodmodel.period_lengths_np(blocks["a stretch holds suffix 0"], p)[0][0] == 30000


def test_premises_of_the_random_blocks():
    for it in range(60):
        T, sp, periods = cases.random_block(it)
        assert T.size <= (1 << 20) and sp in (1, 8) and 2 <= len(periods) <= 3
        assert not any(a != b and a % b == 0 for a in periods for b in periods)
        longest_run, proper = cases.facts(T, periods)
        assert all(proper[p] >= (1 << 15) - p for p in periods), (it, periods, proper)
        assert it % 3 or longest_run >= 4096
