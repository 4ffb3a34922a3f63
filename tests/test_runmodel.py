"""tests/runmodel.py (the run rule of the suffix sorter, stated on its own) against sorted(): the named cases with
their premises -- which members meet k >= h, how many rounds with and without the run step -- and a few thousand
random run-structured strings.  No GPU: these pin the model, not the product."""
import math
import random

import pytest

import runmodel


def _want(T):
    T = bytes(T)
    return sorted(range(len(T)), key=lambda s: T[s:])


def _text(n, seed):
    rng = random.Random(seed)
    words = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(1, 8))) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + b" "
    return bytes(out[:n])


DEPTH = 32

# name -> (text, members with k >= DEPTH, rounds with the step at most, rounds without it at least)
ONE_RUN = {
    "zeros_4Ki": (bytes(4096), 4096 - DEPTH + 1, 1, 6),
    "zeros_64Ki": (bytes(65536), 65536 - DEPTH + 1, 1, 11),
    "zeros_with_a_tail": (bytes(4096) + b"tail", 4096 - DEPTH + 1, 1, 6),
    "x_then_zeros": (b"x" * 4096 + bytes(4096), 2 * (4096 - DEPTH + 1), 1, 6),
    "ff_then_terminator": (b"\xff" * 4096 + b"\0", 4096 - DEPTH + 1, 1, 6),
}


@pytest.mark.parametrize("name", sorted(ONE_RUN))
def test_one_run_takes_one_round(name):
    T, members, with_step, without = ONE_RUN[name]
    assert len(runmodel.run_members(T, DEPTH)) == members                   # premise: who takes the run key
    want = _want(T)
    got, rounds, stepped = runmodel.sort_suffixes(T, DEPTH)
    assert got == want and stepped == DEPTH
    plain, plain_rounds, none = runmodel.sort_suffixes(T, DEPTH, runs=False)
    assert plain == want and none == 0
    assert rounds <= with_step and plain_rounds >= without, (rounds, plain_rounds)
    longest = runmodel.run_lengths(T)[1]
    assert plain_rounds >= math.ceil(math.log2(longest / DEPTH))            # doubling alone: log2(run / depth) rounds


def test_text_with_an_embedded_run():
    T = _text(3000, 1) + bytes(20000) + _text(3000, 2)
    want = _want(T)
    assert len(runmodel.run_members(T, DEPTH)) == 20000 - DEPTH + 1
    got, rounds, stepped = runmodel.sort_suffixes(T, DEPTH)
    plain, plain_rounds, _ = runmodel.sort_suffixes(T, DEPTH, runs=False)
    assert got == want and plain == want and stepped == DEPTH
    assert rounds <= 3 and plain_rounds >= 9, (rounds, plain_rounds)


@pytest.mark.parametrize("name,T", [("period_9", b"abcabcabd" * 2000), ("repeated_8_times", _text(2500, 3) * 8)])
def test_periods_and_copies_gain_nothing(name, T):
    """Periods above one and whole copies are not the rule's: no member meets k >= h, no run step, the plain rounds."""
    assert runmodel.run_members(T, DEPTH) == []
    got, rounds, stepped = runmodel.sort_suffixes(T, DEPTH)
    plain, plain_rounds, _ = runmodel.sort_suffixes(T, DEPTH, runs=False)
    assert got == _want(T) and plain == got
    assert stepped == 0 and rounds == plain_rounds and rounds >= 9, (rounds, plain_rounds)


def test_types_and_ties():
    """x c^L y for x, y below / above / absent; equal runs with different tails, with tails that share a long prefix;
    runs that differ by one; the smallest byte's run ending the text."""
    c, L = 0x50, 300
    run = bytes([c]) * L
    cases = []
    for x in (b"", b"\x10", b"\x90"):
        for y in (b"", b"\x10", b"\x90"):
            cases.append(x + run + y)
            cases.append(b"filler" + x + run + y + b"more filler")
    cases.append(run + b"\x10" + run + b"\x90" + run + b"\x11")
    for shared in (1, 100, 2000):
        tail = _text(shared, 7)
        cases.append(run + tail + b"a" + run + tail + b"b" + run + tail)
    cases.append(run + b"\x90" + run + bytes([c]) + b"\x10" + run[:-1])
    cases.append(b"abc" + bytes(400))
    cases.append(bytes(400) + b"abc" + bytes(200) + b"abd" + bytes(300))
    for T in cases:
        for others in ("lookup", "alone"):
            got, rounds, stepped = runmodel.sort_suffixes(T, 8, others=others)
            plain, plain_rounds, _ = runmodel.sort_suffixes(T, 8, runs=False)
            assert got == _want(T) and plain == got
            assert stepped == 8 and rounds <= plain_rounds + 1


def test_gate_around_the_depth():
    """Runs of d - 1, d and d + 1 bytes: only a run of at least d has members with k >= d."""
    for d in (4, 16, 40):
        for L, members in ((d - 1, 0), (d, 2), (d + 1, 4)):
            T = _text(500, d) + b"\x01" * L + _text(500, d + 1) + b"\x01" * L + b"z"
            assert len(runmodel.run_members(T, d)) == members
            got, rounds, stepped = runmodel.sort_suffixes(T, d)
            plain, plain_rounds, _ = runmodel.sort_suffixes(T, d, runs=False)
            assert got == _want(T) and plain == got
            if members == 0:
                assert stepped == 0 and rounds == plain_rounds
            else:
                assert stepped == d and rounds <= plain_rounds + 1


def test_random_run_structured_strings():
    rng = random.Random(20240611)
    worst = 0
    for it in range(3000):
        sigma = rng.choice([1, 2, 3, 4, 29])
        T = bytearray()
        for _ in range(rng.randint(1, 12)):
            T += bytes([rng.randrange(sigma)]) * rng.choice([1, 2, 3, 7, 8, 9, 31, 33, rng.randint(1, 200)])
        if it % 3 == 0:
            T = T * rng.choice([2, 3])
        T = bytes(T[:600])
        depth = rng.choice([1, 2, 4, 8, 32, 40])
        step_round = rng.choice([0, 1, 2])
        others = rng.choice(["lookup", "alone"])
        want = _want(T)
        got, rounds, stepped = runmodel.sort_suffixes(T, depth, step_round=step_round, others=others)
        assert got == want, (it, T, depth, step_round, others)
        plain, plain_rounds, _ = runmodel.sort_suffixes(T, depth, runs=False)
        assert plain == want
        if not stepped:
            assert rounds == plain_rounds
        worst = max(worst, rounds - plain_rounds)
    assert worst <= 1, worst                                 # never more than one round beyond the plain sorter
