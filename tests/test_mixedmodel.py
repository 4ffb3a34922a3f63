"""tests/mixedmodel.py held to sorted(), to the models it is built on and to its numpy twin, and the premises of the blocks
in tests/mixedcases.py (no GPU, no library)."""
import numpy as np
import pytest

import mixedcases as mc
import mixedmodel as mm
import periodcases as pc
import periodmodel
import runmodel

DEPTHS = (1, 2, 3, 4, 5, 6, 7, 8)


def _sorted(T):
    T = bytes(T)
    return sorted(range(len(T)), key=lambda s: T[s:])


def test_the_model_sorts_and_costs_at_most_one_round_more():
    """Runs, stretches, units a...ab, noise, sigma 2 ... 5, depths 1 ... 8, p on both sides of the depth: the order is
    sorted()'s, and the rounds are at most the one-step sorter's and one more."""
    two = fewer = below = above = inner = 0
    for seed in range(260):
        T, p = mc.model_text(seed)
        want = _sorted(T)
        k1, _ = runmodel.run_lengths(T)
        for depth in DEPTHS:
            order, rounds, steps = mm.sort_suffixes(T, p, depth)
            assert order == want, (seed, p, depth)
            base, base_rounds, _ = mm.one_step(T, p, depth)
            assert base == want and rounds <= base_rounds + 1, (seed, p, depth, rounds, base_rounds)
            assert len(steps) <= 2 and all(at >= q for q, at in steps), (seed, p, depth, steps)
            two += len(steps) == 2
            fewer += rounds < base_rounds
            below += p <= depth and bool(steps)
            above += p > depth and bool(steps)
            inner += len(steps) == 2 and any(depth <= k < p for k in k1)
    print("%d cases with two steps, %d with fewer rounds than one step takes" % (two, fewer))
    assert two >= 200 and fewer >= 200 and below >= 100 and above >= 200 and inner >= 100, (two, fewer, below, above, inner)


def test_without_a_long_run_it_is_the_period_model():
    seen = 0
    for seed in range(300):
        T, p = mc.model_text(seed)
        _, longest_run = runmodel.run_lengths(T)
        for depth in (4, 8, 16, 40):
            if longest_run > depth:
                continue
            # (the period model gates on the longest stretch, this one on the longest proper stretch: the same step
            # wherever both open or both stay shut)
            kp, longest = periodmodel.period_lengths(T, p)
            if (longest > max(depth, p)) != (mm.longest_proper(T, p) > max(depth, p)) or p > depth:
                continue
            want = periodmodel.sort_suffixes(T, p, depth)
            got = mm.sort_suffixes(T, p, depth)
            assert got[0] == want[0] and got[1] == want[1] and got[2] == ([(p, want[2])] if want[2] else []), (seed, p, depth)
            seen += 1
    assert seen >= 100, seen


def test_without_a_stretch_it_is_the_run_model():
    seen = 0
    for seed in range(200):
        T = mc.runs_only_text(seed)
        _, longest_run = runmodel.run_lengths(T)
        for p in (2, 3, 7):
            for depth in (1, 2, 4):
                if mm.longest_proper(T, p) > max(2 * depth, p) or longest_run <= depth:
                    continue
                want = runmodel.sort_suffixes(T, depth)
                got = mm.sort_suffixes(T, p, depth)
                if p <= depth and mm.longest_proper(T, p) > depth:
                    continue
                assert got[0] == want[0] == _sorted(T) and got[1] == want[1] and got[2] == [(1, want[2])], (seed, p, depth, got[2])
                seen += 1
    assert seen >= 200, seen


def test_statement_a_position_by_position():
    """k_p[s] = k_1[s] and the same type wherever k_1[s] >= p."""
    held = 0
    for seed in range(400):
        T, _ = mc.model_text(seed, 150)
        k1, _ = runmodel.run_lengths(T)
        for p in (2, 3, 4, 7, 13, 20):
            assert mm.statement_a(T, p) == [], (seed, p)
            held += sum(1 for k in k1 if k >= p)
    assert held >= 10000, held


def test_the_numpy_twin():
    for seed in range(120):
        T, p = mc.model_text(seed)
        A = np.frombuffer(T, np.uint8)
        assert mm.longest_proper_np(A, p) == mm.longest_proper(T, p)
        for depth in (1, 3, 8):
            order, rounds, steps = mm.sort_suffixes(T, p, depth)
            got = mm.sort_suffixes_np(A, p, depth)
            assert got[0].tolist() == order and got[1] == rounds and got[2] == steps, (seed, p, depth, got[1:], rounds, steps)
            base = mm.one_step(T, p, depth)
            got = mm.sort_suffixes_np(A, p, depth, mixed=False)
            assert got[0].tolist() == base[0] and got[1] == base[1] and got[2] == base[2], (seed, p, depth, got[1:], base[1:])
    for n in (0, 1, 2):
        assert mm.longest_proper_np(np.zeros(n, np.uint8), 3) == mm.longest_proper(bytes(n), 3) == 0


# ---- the premises of tests/mixedcases.py ---------------------------------------------------------

@pytest.mark.parametrize("p", [q for q in pc.PERIODS if q > 1])
def test_premises_of_the_pass_blocks(p):
    blocks = dict(mc.proper_blocks(p))
    T = blocks["the longest stretch is a run"]
    k, longest = periodmodel.period_lengths_np(T, p)
    assert 0 < mm.longest_proper_np(T, p, k) < longest
    for delta in (-1, 0, 1):
        T = blocks["a run of p %+d bytes beside a stretch" % delta]
        assert max(p + delta, 1) in periodmodel.period_lengths_np(T, 1)[0].tolist()
    for name, s in (("chunk", pc.TILE + 4096 + 63), ("wave", pc.TILE + 4095), ("tile", 2 * pc.TILE - 1), ("n - 2", 3 * pc.TILE + 998)):
        T = blocks["the proper position on the last byte of a %s" % name]
        assert np.flatnonzero(T[:-1] != T[1:]).tolist() == [s] and (s % 64 == 63 or s == T.size - 2)
        assert mm.longest_proper_np(T, p) == periodmodel.period_lengths_np(T, p)[0][s] > 0
    assert mm.longest_proper_np(blocks["all equal"], p) == 0
    assert any(T.size <= p for T in blocks.values())


def test_premises_of_the_step_blocks():
    for p in (2, 9, 64, 300):
        for run in (1 << 16, 1 << 18):
            for stretch in (1 << 16, 1 << 18):
                d = mc.run_and_stretch(p, run, stretch)
                for T in (d, d[::-1]):
                    longest_run, proper = mc.facts(T, p)
                    assert longest_run == run and stretch - p <= proper <= stretch + p, (p, run, stretch, longest_run, proper)
    for p, lo in ((64, 16), (300, 16)):
        d = mc.short_runs_beside_stretches(p, lo)
        k1 = periodmodel.period_lengths_np(d, 1)[0]
        starts = np.flatnonzero(np.r_[True, d[1:] != d[:-1]])
        lens = k1[starts]
        assert ((lens >= lo) & (lens < p)).sum() >= 7 and lens.max() == 8192, (p, lens.max())
        assert mc.facts(d, p)[1] >= 40000 - p
    for p in (3, 9, 64):
        for name, d in mc.seam_blocks(p):
            longest_run, proper = mc.facts(d, p)
            assert longest_run >= 5000 and proper >= 20000 - p, (p, name, longest_run, proper)


def test_premises_of_the_random_blocks():
    """Every block of the randomised case holds a run of 4096 bytes or more and a proper stretch of 2^15 or more, whose
    period wins the vote with max(256, n / 64) votes or more at the depths the rounds may begin at."""
    for it in range(60):
        d, sp, p = mc.random_block(it)
        assert d.size <= (1 << 20) and sp in (1, 8)
        for T in (d, d[::-1]):
            longest_run, proper = mc.facts(T, p)
            assert longest_run >= 4096 and proper >= (1 << 15) - p, (it, p, longest_run, proper)
        if it % 6 == 0:
            for depth in (4, 8):
                v = mc.votes_np(d[::-1] if it % 12 else d, depth)
                assert max(v, key=v.get) == p and v[p] >= max(256, d.size // 64), (it, p, depth, sorted(v.items(), key=lambda x: -x[1])[:3])
