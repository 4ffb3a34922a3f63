"""The long periods' model (tests/longperiodmodel.py) and the premises of the GPU tests' blocks (tests/longcases.py),
without a GPU: the period rule of tests/periodmodel.py at p = 4097, 5000 and 8192 against sorted(), the finder's contract
against a count by hand, the probe and both maxima against loops, and for every named block the period, the longest
stretch, the votes and the rounds the GPU tests expect."""
import numpy as np
import pytest

import longcases as lc
import longperiodmodel as lm
import periodcases as pc
import periodmodel as pm


# ---- the rule -------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [4097, 5000, 8192])
def test_the_rule_holds_above_4096(p):
    """Prefix doubling with the deferred step of period p gives sorted()'s order, takes the step at the first depth that
    reaches p and saves rounds; blocks of at most 2^17 bytes."""
    # (s and s + p share k_p[s] - p characters: a stretch of p + the step's depth + 400 still ties 400 suffixes there)
    T = bytes(pc.cat(pc.filler(700, p), pc.stretch(p, p + lm.step_depth(p, 1) + 400), [0], pc.filler(500, p + 1), pc.stretch(p, p + 900, 0, 7), [255]))
    assert len(T) <= 1 << 17
    want = sorted(range(len(T)), key=lambda s: T[s:])
    order, rounds, stepped = pm.sort_suffixes(T, p, 1, True)
    plain, plain_rounds, never = pm.sort_suffixes(T, p, 1, False)
    assert order == want and plain == want
    assert stepped == lm.step_depth(p, 1) and p <= stepped < 2 * p and never == 0
    # (a stretch this short is through one doubling later: the step costs no round here, and saves them on longer ones)
    assert rounds <= lm.step_rounds(p, 1) + 3 and rounds <= plain_rounds, (rounds, plain_rounds)
    assert plain_rounds >= lm.plain_rounds(np.frombuffer(T, np.uint8), p, 1)


def test_round_formulas():
    assert [lm.step_rounds(p, 64) for p in (9, 64, 65, 128, 129, 4097, 8192, 65536)] == [0, 0, 1, 1, 2, 7, 7, 10]
    assert [lm.step_depth(p, 48) for p in (48, 49, 4097, 65537)] == [48, 96, 6144, 98304]
    assert lm.probe_span(4097, 64) == (8 * 4097 - 4097) // 2 and lm.need_of(1 << 20) == 16384 and lm.need_of(100) == 256


# ---- the finder -----------------------------------------------------------------------------

def _brute(ks, vs, kmask, need, k1=None):
    table = {}
    for i in range(len(ks) - 1):
        if (int(ks[i]) ^ int(ks[i + 1])) & kmask:
            continue
        a, b = int(vs[i]), int(vs[i + 1])
        d = abs(a - b)
        if d < 2 or d > 1 << 24 or (k1 is not None and int(k1[min(a, b)]) > d):
            continue
        table[d] = table.get(d, 0) + 1
    good = sorted(((v, d) for d, v in table.items() if v >= need), key=lambda vd: (-vd[0], vd[1]))
    return [(d, v) for v, d in good[:8]]


@pytest.mark.parametrize("seed", range(6))
def test_candidates_against_a_count_by_hand(seed):
    rng = np.random.default_rng([41, seed])
    m = 6000
    far = [] if seed % 2 else [1 << 24, (1 << 24) + 1]          # (with k1[]: positions below 2^21, so that k1[] stays small)
    size = 1 << 21 if seed % 2 else 1 << 26
    dist = rng.choice([3, 4096, 4097, 8191, 8192, 70000] + far, m)
    vs = np.cumsum(dist) % size
    ks = np.cumsum(rng.random(m) < 0.02).astype(np.uint64) | (rng.integers(0, 4, m).astype(np.uint64) << np.uint64(56))
    k1 = rng.choice([1, 5000, 100000], size).astype(np.uint32) if seed % 2 else None
    kmask = (1 << 56) - 1
    for need in (1, 200, 600):
        assert lm.candidates((ks, vs), kmask, need, k1) == _brute(ks, vs, kmask, need, k1), (seed, need)


def test_probe_and_maxima_against_loops():
    p, n = 4097, 40000
    T = lc.noise(n, 1).copy()
    T[5000:5000 + 20000] = pc.stretch(p, 20000)
    k, longest, proper = lm.lengths(T, p)
    kk, ll = pm.period_lengths(bytes(T), p)
    assert list(k) == kk and longest == ll
    assert proper == max(kk[s] for s in range(n - 1) if T[s] != T[s + 1])
    brk = [q >= p and T[q] != T[q - p] for q in range(n)]
    for span in (1, 100, 5000, 7951, 7952, 14339):
        want = any(not any(brk[x:x + span]) for x in range(p, n - span + 1, span) if n > p + span)
        assert lm.probe(T, p, span) == want, span


# ---- the premises of the GPU tests' blocks ----------------------------------------------------

def _premise(d, p, h_first=8):
    """(the longest stretch, the votes of p in a list sorted to 8 characters, need)"""
    longest = lm.lengths(d, p)[1]
    votes = lm.vote_table(*lm.sorted_list_np(d, 8), (1 << 64) - 1).get(p, 0)
    return longest, votes, lm.need_of(d.size)


@pytest.mark.parametrize("p,inside", lc.ONE_STRETCH)
def test_one_stretch_premise(p, inside):
    d = lc.one_stretch(p, inside)
    longest, votes, need = _premise(d, p)
    assert 1 << 20 <= d.size <= 4 << 20 and 16 * p <= longest <= 16 * p + 8 and votes >= need, (d.size, longest, votes, need)
    assert lm.takes_step(d, p, 64) and lm.probe(d, p, lm.probe_span(p, 64))
    assert lm.candidates(lm.sorted_list_np(d, 8), (1 << 64) - 1, need)[0][0] == p
    assert lm.plain_rounds(d, p, 64) >= lm.step_rounds(p, 64) + 3


@pytest.mark.parametrize("p", [4097, 8192])
def test_tie_and_worth_premises(p):
    for what, d in lc.tie_blocks(p):
        longest, votes, need = _premise(d, p)
        assert longest >= 9 * p + 5 and votes >= need and lm.takes_step(d, p, 64), (what, longest, votes, need)
    S = pc.stretch(p, 9 * p + 5)
    nxt = int(pc.unit(p, 0)[(9 * p + 5) % p])
    assert 1 <= nxt - 1 and nxt + 1 <= 255                  # a smaller and a larger byte exist: both types
    two = dict(lc.tie_blocks(p))["equal (type, k) from 2 stretches"]
    k = lm.lengths(two, p)[0]
    assert int((k == k.max()).sum()) >= 1 and int((k >= 9 * p).sum()) >= 2   # two stretches of one length: ties by the tail's rank
    for delta in (-1, 0, 1):
        d = lc.worth_block(p, delta)
        longest, votes, need = _premise(d, p)
        assert longest == 8 * p + delta and votes >= need and 8 * p <= d.size, (delta, longest, votes, need)
        assert lm.probe(d, p, lm.probe_span(p, 64)), delta                  # the probe lets all three through: the pass decides
        assert lm.takes_step(d, p, 64) == (delta >= 0), delta
    assert S.size == 9 * p + 5


def test_forced_division_and_multi_premises():
    p = 4999
    d = lc.forced_block(p)
    assert lm.lengths(d, p)[1] in (3 * p, 3 * p + 1) and not lm.takes_step(d, p, 64)      # votes would not buy it
    assert lm.lengths(d, p)[1] > lm.step_depth(p, 64)                                     # ... and the gate lets a named period through
    for q in (4100, 8192):
        d = lc.division_block(q)
        longest, votes, need = _premise(d, q)
        assert votes >= need and lm.takes_step(d, q, 64)
        for f in (2, 5, 41):
            if q % f == 0:
                assert lm.lengths(d, q // f)[1] < longest                                 # no divisor keeps the stretch: q stays
    d = lc.long_and_short()
    table = lm.vote_table(*lm.sorted_list_np(d, 8), (1 << 64) - 1)
    need = lm.need_of(d.size)
    assert table.get(9, 0) >= need and table.get(5000, 0) >= need and 8 * 5000 <= d.size
    assert lm.lengths(d, 5000)[2] >= 8 * 5000 and lm.lengths(d, 9)[2] >= 8 * 64


@pytest.mark.parametrize("q", sorted(lc.MULTIPLE_OF))
def test_a_winner_that_is_a_multiple_premise(q):
    """In window_order_list() the votes of multiple_block(q) name lcm(q, 256) = 262 400, above 4096 for both q; it passes
    the probe and the worth test, and the division brings it down to q -- 4100, a long period, and 1025, a short one.
    In position order the winner is q and the division tries q's prime factors in vain."""
    import math
    d = lc.multiple_block(q)
    w = lc.MULTIPLE_OF[q]
    assert w == q * 256 // math.gcd(q, 256) == 262400 and 8 * w <= d.size
    need = lm.need_of(d.size)
    cands = lm.candidates(lm.window_order_list(d, 8), (1 << 64) - 1, need)
    assert cands and cands[0][0] == w and cands[0][1] >= need, cands[:3]
    assert not [c for c in cands if c[0] <= 4096], cands                      # the short finder alone finds nothing
    longest = lm.lengths(d, w)[1]
    assert longest >= 3 << 20 and longest >= 8 * w and lm.probe(d, w, lm.probe_span(w, 64))
    left, tried = lm.divided(d, w)
    assert left == q and w // 2 in tried and len(tried) >= 8, (left, tried)
    assert lm.takes_step(d, q, 64)
    assert lm.candidates(lm.sorted_list_np(d, 8), (1 << 64) - 1, need)[0][0] == q and lm.divided(d, q)[0] == q


def test_back_to_back_premise():
    d = lc.back_to_back()
    p = 1 << 16
    longest, votes, need = _premise(d, p)
    assert d.size == 2 << 20 and longest == d.size and votes >= need and lm.takes_step(d, p, 64)
    assert lm.candidates(lm.sorted_list_np(d, 8), (1 << 64) - 1, need)[0][0] == p
    assert lm.step_rounds(p, 64) == 10 and lm.plain_rounds(d, p, 64) >= 15


def test_random_blocks_premise():
    """Every one of the 40 has a stretch of at least 9 p, p in 4097 ... 40 000, that the votes buy and the rule takes."""
    for it in range(40):
        d, p, L = lc.random_block(it)
        assert 4097 <= p <= 40000 and L >= 9 * p and 8 * p <= d.size <= 1 << 20
        longest = lm.lengths(d, p)[1]
        # inside the stretch s and s + p are neighbours of one group at any depth up to p: L - 2 p votes at the least
        assert longest >= L and L - 2 * p >= lm.need_of(d.size) and lm.takes_step(d, p, 4096), (it, p, L, longest)
        if it % 8 == 0:
            assert _premise(d, p)[1] >= L - p - 8, it


def test_controls_hold_no_long_period():
    for what, d in lc.controls():
        table = lm.vote_table(*lm.sorted_list_np(d, 8), (1 << 64) - 1)
        assert not [v for q, v in table.items() if q > 4096 and v >= lm.need_of(d.size)], what


def test_seam_blocks():
    for p in lc.LENGTH_PERIODS:
        s = lc.seams(p)
        assert s["load"] % 16 == 0 and s["thread"] % 64 == 0 and s["wave"] % 4096 == 0 and s["tile"] % lc.TILE == 0
        assert all(q >= p for q in s.values()) and p < lc.LENGTHS_N
    T, at = lc.seam_block(4097, 0, 1 << 18)
    assert set(at) <= set(np.flatnonzero(lm.breaks_of(T, 4097)).tolist())
