"""tests/periodmodel.py (the period rule of the suffix sorter, stated on its own) against sorted() and against
tests/runmodel.py, and the premises of the GPU tests' named blocks (tests/periodcases.py): each has the edge it is
named for, proved with the model alone.  No GPU: these pin the model and the cases, not the product."""
import math
import random

import numpy as np
import pytest

import periodcases as pc
import periodmodel
import runmodel
import test_runmodel


def _want(T):
    T = bytes(T)
    return sorted(range(len(T)), key=lambda s: T[s:])


# ---- p = 1 is the run rule ------------------------------------------------------------------

def _run_cases():
    out = [T for T, _, _, _ in test_runmodel.ONE_RUN.values()]
    out.append(test_runmodel._text(3000, 1) + bytes(20000) + test_runmodel._text(3000, 2))
    out += [b"abcabcabd" * 2000, test_runmodel._text(2500, 3) * 8]
    return out


def test_period_one_is_the_run_model():
    for T in _run_cases():
        assert periodmodel.period_lengths(T, 1) == runmodel.run_lengths(T)
        k = runmodel.run_lengths(T)[0]
        for s in range(0, len(T), 97):
            assert periodmodel.falling(T, k, s, 1) == runmodel.falling(T, k, s)
            assert periodmodel.period_key(T, k, s, 1) == runmodel.run_key(T, k, s)
        for others in ("lookup", "alone"):
            got = periodmodel.sort_suffixes(T, 1, test_runmodel.DEPTH, others=others)
            ref = runmodel.sort_suffixes(T, test_runmodel.DEPTH, others=others)
            assert got[0] == ref[0] and got[2] == ref[2], (len(T), others, got[1:], ref[1:])
            assert got[1] == ref[1]


def test_numpy_lengths_are_the_model():
    rng = random.Random(5)
    for it in range(300):
        n = rng.choice([1, 2, 3, 17, 64, 65, 300])
        T = bytes(rng.randrange(rng.choice([1, 2, 3])) for _ in range(n))
        p = rng.choice([1, 2, 3, 7, 64, 65, 400])
        k, longest = periodmodel.period_lengths(T, p)
        k2, longest2 = periodmodel.period_lengths_np(np.frombuffer(T, np.uint8), p)
        assert list(k2) == k and longest2 == longest, (T, p)
        assert all(k[s] == n - s for s in range(max(0, n - p), n))     # nothing breaks behind n - p


# ---- the model is the suffix order ----------------------------------------------------------

def _stretch_text(rng, sigma, periods, n):
    out = bytearray()
    while len(out) < n:
        if rng.random() < 0.3:
            out += bytes(1 + rng.randrange(sigma) for _ in range(rng.randint(1, 12)))
        else:
            p = rng.choice(periods)
            u = bytes(1 + rng.randrange(sigma) for _ in range(p))
            L = rng.choice([p, p + 1, 2 * p, 2 * p + 1, 3 * p - 1, rng.randint(1, 150)])
            out += (u * (L // p + 1))[:L]
    return bytes(out[:n])


def test_random_matrix_against_sorted():
    """Periods 2 ... 33, alphabets of 2, 3, 4 and 200 symbols, stretches of the chosen and of other periods mixed with
    noise, depths 1, 2, 4, p, p + 1 and 16, with and without a terminator, both treatments of the other members."""
    rng = random.Random(20250101)
    stepped_at = {}
    for it in range(1500):
        p = rng.randint(2, 33)
        sigma = rng.choice([2, 3, 4, 200])
        periods = [p] * 3 + [rng.randint(1, 33), 1]
        T = _stretch_text(rng, sigma, periods, rng.choice([40, 150, 400]))
        if it % 2:
            T += b"\0"
        depth = rng.choice([1, 2, 4, p, p + 1, 16])
        others = rng.choice(["lookup", "alone"])
        want = _want(T)
        got, rounds, stepped = periodmodel.sort_suffixes(T, p, depth, others=others)
        assert got == want, (it, T, p, depth, others)
        plain, plain_rounds, none = periodmodel.sort_suffixes(T, p, depth, step=False)
        assert plain == want and none == 0
        if stepped:
            assert stepped >= p and (stepped == depth or stepped < 2 * p), (stepped, p, depth)
            stepped_at[stepped > depth] = stepped_at.get(stepped > depth, 0) + 1
        else:
            assert rounds == plain_rounds
    assert stepped_at.get(False, 0) > 100 and stepped_at.get(True, 0) > 100, stepped_at     # first-round and deferred steps


@pytest.mark.parametrize("wrong", [4, 9])
def test_a_wrong_period_costs_rounds_never_the_order(wrong):
    rng = random.Random(wrong)
    for it in range(60):
        u = bytes(rng.randrange(1, 4) for _ in range(5)) + b"\x09"          # period 6, primitive
        T = _stretch_text(rng, 3, [1], 30) + u * rng.randint(3, 40) + _stretch_text(rng, 3, [2], 30) + u * rng.randint(3, 25)
        for depth in (1, 4, 16):
            for others in ("lookup", "alone"):
                got, _, _ = periodmodel.sort_suffixes(T, wrong, depth, others=others)
                assert got == _want(T), (it, T, wrong, depth, others)


@pytest.mark.parametrize("p", [2, 3, 9, 33, 64, 100])
def test_one_stretch_ends_within_the_bound(p):
    """A block that is one stretch: ceil(log2(max(1, p / depth))) ordinary rounds until the depth reaches p, the step,
    and at most one round behind it."""
    rng = random.Random(p)
    u = bytes(rng.randrange(1, 250) for _ in range(p - 1)) + b"\xfb"
    T = (u * (3000 // p + 2))[:3000]
    for depth in (1, 4, 16, 64):
        got, rounds, stepped = periodmodel.sort_suffixes(T, p, depth)
        assert got == _want(T) and stepped >= p
        assert rounds <= math.ceil(math.log2(max(1, p / depth))) + 2, (p, depth, rounds)
        _, plain_rounds, _ = periodmodel.sort_suffixes(T, p, depth, step=False)
        assert plain_rounds >= math.floor(math.log2(3000 / max(depth, p))), (p, depth, plain_rounds)


def test_votes_find_the_period():
    T = b"abcabcabd" * 3000
    v4 = periodmodel.votes(T, 4)
    assert v4[9] == 14992 and v4[3] == 6000 and max(v4, key=v4.get) == 9
    v8 = periodmodel.votes(T, 8)
    assert set(v8) == {9}
    assert periodmodel.votes(bytes(5000), 8) == {}                          # a run votes for distance 1, which is no vote
    noise = bytes(random.Random(1).randrange(256) for _ in range(20000))
    assert sum(periodmodel.votes(noise, 4).values()) < 20000 // 64


# ---- the premises of the GPU tests' blocks --------------------------------------------------

@pytest.mark.parametrize("p", [2, 9, 64, 257, 4096])
def test_placed_breaks_are_the_only_breaks(p):
    """with_breaks() makes exactly the asked positions breaks, so the seam blocks have a break at -1 / 0 / +1 around
    every seam (and exactly p before it) and no other; k is n - s in a block that is one stretch."""
    n = pc.SEAM_N
    S = pc.stretch(p, n)
    k, longest = periodmodel.period_lengths_np(S, p)
    assert longest == n and (k == n - np.arange(n)).all()
    for breaks in (pc.seam_breaks(p, -1), pc.seam_breaks(p, 0), pc.seam_breaks(p, 1), pc.before_seam_breaks(p), pc.spaced_breaks(p)):
        T = pc.with_breaks(S, p, breaks)
        found = np.flatnonzero(T[p:] != T[:-p]) + p
        assert list(found) == sorted(breaks), (p, breaks, found)
    assert len(pc.seam_breaks(p, 0)) == len(pc.SEAMS) and pc.SEAM_N - 1 in pc.seam_breaks(p, 0)
    gaps = np.diff(pc.spaced_breaks(p))
    assert {max(p - 1, 1), p, p + 1} <= set(int(g) for g in gaps)
    for q in pc.SEAMS.values():                                           # the seams are what they are named for
        assert q % 16 == 0 or q == pc.SEAM_N - 1
    assert pc.SEAMS["load"] % 64 and pc.SEAMS["thread"] % 64 == 0 and pc.SEAMS["thread"] % 4096
    assert pc.SEAMS["wave"] % 4096 == 0 and pc.SEAMS["wave"] % pc.TILE and pc.SEAMS["tile"] % pc.TILE == 0


@pytest.mark.parametrize("p", [2, 3, 9, 64])
def test_tie_blocks_hold_their_ties(p):
    """Small versions of the tie blocks: falling and rising members, (type, k) shared by as many stretches as the name
    says, and the model sorts them."""
    for name, T in pc.tie_blocks(p, 40 * p if p > 9 else 150):
        T = bytes(T)
        k, _ = periodmodel.period_lengths(T, p)
        h = 2 * p
        keys = {}
        for s in range(len(T)):
            if k[s] >= h:
                keys.setdefault(periodmodel.period_key(T, k, s, p), []).append(s)
        types = {key[0] for key in keys}
        most = max(len(v) for v in keys.values())
        if "below, above" in name or "rotations" in name or "each other" in name:
            assert types == {0, 1}, (name, types)
        if name.startswith("equal"):
            copies = int(name.split()[4])
            assert most >= copies // 2, (name, most)                       # (every other stretch ends the same way)
        for others in ("lookup", "alone"):
            got, _, stepped = periodmodel.sort_suffixes(T, p, h, others=others)
            assert got == _want(T) and stepped == h, (p, name, others)
    T = bytes(pc.nonprimitive_block(200))
    got, _, stepped = periodmodel.sort_suffixes(T, 4, 8)
    assert got == _want(T) and stepped == 8
    assert periodmodel.period_lengths(T, 2)[1] == periodmodel.period_lengths(T, 4)[1] >= 200         # abab is 4-periodic as well


def test_gate_blocks_hold_exactly_the_planted_stretch():
    for p in (2, 3):
        plain = periodmodel.period_lengths_np(pc.gate_block(p, 0), p)[1]
        assert plain <= p + 3, plain                                       # noise: k_p is p plus the few bytes that agree by chance
        for planted in (7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65):
            assert periodmodel.period_lengths_np(pc.gate_block(p, planted), p)[1] == planted
            assert pc.gate_block_longest(p, planted) <= p + 3


def test_units_of_five_symbols():
    for p in (5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 65):
        u = pc.unit_of_five(p)
        assert sorted(set(u.tolist())) == [65, 67, 71, 84, 90] and (u == 90).sum() == 1      # five symbols, primitive
        T = np.tile(u, 70000 // p)
        assert periodmodel.period_lengths_np(T, p)[1] == T.size
        assert all(periodmodel.period_lengths_np(T, q)[1] <= q + p for q in range(1, p))   # no shorter period


def test_random_blocks_mix_periods():
    seen = set()
    for it in range(0, 100, 7):
        d, sp = pc.random_block(it)
        assert 150 <= d.size <= 300000 and sp in (1, 2, 8, 256)
        for p in (1, 2, 9, 64):
            if periodmodel.period_lengths_np(d, p)[1] > 4 * p + 64:
                seen.add(p)
    assert seen == {1, 2, 9, 64}, seen
