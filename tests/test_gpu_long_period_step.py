"""The period step at periods above 4096 on the GPU (-m gpu; BWTC_HIP_LONG_PERIODS=1): the blocks of tests/longcases.py,
every result -- bytes, LF powers, freqs -- against oracle.oracle_bwt_block; the route (bwtc_hip_stats.route bit 11),
bwtc_hip_period_get, the schedule and the rounds as tests/longperiodmodel.py says: from a first round at depth d (the
sorter's debug line) the step of period p runs at the first of d, 2 d, 4 d ... that reaches p, and the block is through
at most 3 rounds behind the step_rounds(p, d) that double before it -- the margin of tests/test_gpu_period_step.py.
A switch is read when a context is made: every test opens one context with the switch and one without, which must give
the same bytes, a clear bit, no long period and the rounds of plain doubling.

On a sorter that ignores the switch the asserts on `route & 2048` and on the rounds fail."""
import contextlib
import re

import numpy as np
import pytest

import longcases as lc
import longperiodmodel as lm

pytestmark = pytest.mark.gpu

LONG_BIT, PERIOD_BIT, MULTI_BIT, COPY_BIT = 2048, 256, 512, 1024
STEP_LINE = re.compile(r"periods: period (\d+) with (\d+) votes, longest stretch (\d+), the rounds begin at depth (\d+): period step at depth (\d+)")
RUNS_LINE = re.compile(r"runs: longest run (\d+), the rounds begin at depth (\d+)")
SIZE = 2 << 20


@contextlib.contextmanager
def _contexts(monkeypatch, size, extra=""):
    """(a context with BWTC_HIP_LONG_PERIODS=1, one without), both with the switches of `extra`."""
    from bwtc_amd import hip
    names = []
    for one in extra.split(","):
        if one:
            name, value = one.split("=")
            monkeypatch.setenv(name, value)
            names.append(name)
    monkeypatch.delenv("BWTC_HIP_LONG_PERIODS", raising=False)
    ctx_off = hip.Context(0, size)
    monkeypatch.setenv("BWTC_HIP_LONG_PERIODS", "1")
    ctx_on = hip.Context(0, size)
    monkeypatch.delenv("BWTC_HIP_LONG_PERIODS")
    for name in names:
        monkeypatch.delenv(name)
    try:
        yield ctx_on, ctx_off
    finally:
        ctx_on.close()
        ctx_off.close()


def _same(ctx, d, sp, want, what):
    got = ctx.bwt_block(d, sp)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[2] == want[2]).all(), what
    return ctx.stats()


def _said(ctx, d, sp, want, what, monkeypatch, capfd):
    """_same() with the sorter's debug lines -> (stats, the depth the rounds begin at or 0, the step's line or None)."""
    monkeypatch.setenv("BWTC_HIP_DEBUG", "1")
    capfd.readouterr()
    try:
        st = _same(ctx, d, sp, want, what)
    finally:
        monkeypatch.delenv("BWTC_HIP_DEBUG")
    err = capfd.readouterr().err
    runs, steps = RUNS_LINE.findall(err), STEP_LINE.findall(err)
    depth = int(runs[0][1]) if runs else 0
    line = None
    for p, votes, longest, d0, at in steps:
        line = dict(p=int(p), votes=int(votes), longest=int(longest), depth=int(d0), at=int(at))
    return st, depth, line


def _stepped(ctx, ctx_off, d, p, sp, oracle, monkeypatch, capfd, what, zeros_off=True):
    """The block takes the step of period p with the switch -- bit 11, period(), schedule(), rounds -- and is the plain
    sorter's without it."""
    want = oracle.oracle_bwt_block(d, sp)
    st, depth, line = _said(ctx, d, sp, want, what, monkeypatch, capfd)
    period, schedule = ctx.period(), ctx.schedule()
    st_off, depth_off, line_off = _said(ctx_off, d, sp, want, (what, "off"), monkeypatch, capfd)
    print("%s: p %d, %d bytes: rounds %d route %#x period %s schedule %s, the rounds begin at depth %d; without: rounds %d route %#x"
          % (what, p, d.size, st.rounds, st.route, period, schedule, depth, st_off.rounds, st_off.route))
    assert st.route & LONG_BIT and st.route & PERIOD_BIT, (what, hex(st.route), period, line)
    assert depth > 0 and line and line["p"] == p and line["depth"] == depth, (what, depth, line)
    at = lm.step_depth(p, depth)
    longest = lm.lengths(d, p)[1]
    assert period[0] == p and period[1] == longest and period[3] == at == line["at"], (what, period, at, longest, line)
    assert [(e[0], e[1]) for e in schedule if e[0] == p] == [(p, at)], (what, schedule)
    assert st.rounds <= lm.step_rounds(p, depth) + 3, (what, st.rounds, depth)
    # without the switch: the parent's sorter
    assert not st_off.route & LONG_BIT and ctx_off.period()[0] <= 4096, (what, hex(st_off.route), ctx_off.period())
    if zeros_off:
        # (no period, no stretch, no step; the third word is the short finder's leader's votes, below the threshold)
        off = ctx_off.period()
        assert (off[0], off[1], off[3]) == (0, 0, 0) and off[2] < lm.need_of(d.size) and not st_off.route & PERIOD_BIT and line_off is None, (what, off, line_off)
    plain = lm.plain_rounds(d, p, depth)
    assert depth_off == depth and plain <= st_off.rounds <= plain + lm.PLAIN_MARGIN, (what, st_off.rounds, plain, depth_off)
    return st, st_off


@pytest.mark.parametrize("p,inside", lc.ONE_STRETCH)
def test_one_stretch(oracle, monkeypatch, capfd, p, inside):
    d = lc.one_stretch(p, inside)
    with _contexts(monkeypatch, d.size) as (ctx, ctx_off):
        for sp in (1, 8):
            st, st_off = _stepped(ctx, ctx_off, d, p, sp, oracle, monkeypatch, capfd, ("one stretch", inside, sp), zeros_off=inside == "random")
        assert ctx.period()[2] >= lm.need_of(d.size)
        assert st.rounds < st_off.rounds, (st.rounds, st_off.rounds)


@pytest.mark.parametrize("p", [4097, 8192])
def test_types_and_ties(oracle, monkeypatch, capfd, p):
    """Stretches that end in a smaller byte, a larger byte, the block's end and each other; equal (type, k) from two and
    three stretches of one unit (ties by the tail's rank); rotations of one unit."""
    with _contexts(monkeypatch, 1 << 20) as (ctx, ctx_off):
        for what, d in lc.tie_blocks(p):
            _stepped(ctx, ctx_off, d, p, 8, oracle, monkeypatch, capfd, (p, what))


@pytest.mark.parametrize("p", [4097, 8192])
def test_the_worth_threshold(oracle, monkeypatch, capfd, p):
    """A longest stretch of 8 p - 1 is refused by the worth test, 8 p and 8 p + 1 take the step."""
    with _contexts(monkeypatch, 1 << 20) as (ctx, ctx_off):
        d = lc.worth_block(p, -1)
        want = oracle.oracle_bwt_block(d, 8)
        st = _same(ctx, d, 8, want, (p, -1))
        st_off = _same(ctx_off, d, 8, want, (p, -1, "off"))
        assert not st.route & (LONG_BIT | PERIOD_BIT) and ctx.period()[0] == 0 and ctx.period()[3] == 0, (hex(st.route), ctx.period())
        assert (st.rounds, st.route, st.active_sum) == (st_off.rounds, st_off.route, st_off.active_sum)
        for delta in (0, 1):
            _stepped(ctx, ctx_off, lc.worth_block(p, delta), p, 8, oracle, monkeypatch, capfd, (p, "worth", delta))


def test_a_named_long_period(oracle, monkeypatch):
    """BWTC_HIP_LONG_PERIOD names a period that the votes would not buy; without the switch it is not read."""
    p = 4999
    d = lc.forced_block(p)
    want = oracle.oracle_bwt_block(d, 8)
    with _contexts(monkeypatch, 1 << 20, "BWTC_HIP_LONG_PERIOD=%d" % p) as (ctx, ctx_off):
        st = _same(ctx, d, 8, want, "named")
        assert st.route & LONG_BIT and ctx.period()[0] == p and ctx.period()[2] == 0 and p <= ctx.period()[3] < 2 * p, (hex(st.route), ctx.period())
        st_off = _same(ctx_off, d, 8, want, "named, off")
        assert not st_off.route & (LONG_BIT | PERIOD_BIT) and ctx_off.period()[0] == 0 and ctx_off.period()[3] == 0, ctx_off.period()
    with _contexts(monkeypatch, 1 << 20) as (ctx, ctx_off):              # not named: the votes do not reach the worth
        st = _same(ctx, d, 8, want, "not named")
        assert not st.route & LONG_BIT, hex(st.route)


@pytest.mark.parametrize("p", [4100, 8192])
def test_the_division_keeps_a_primitive_period(oracle, monkeypatch, capfd, p):
    """p = 2^2 5^2 41 and 2^13: the division tries p / 2, p / 5 and p / 41 (trial passes) and keeps p."""
    with _contexts(monkeypatch, 1 << 20) as (ctx, ctx_off):
        _stepped(ctx, ctx_off, lc.division_block(p), p, 8, oracle, monkeypatch, capfd, ("division", p))


TRIAL_LINE = re.compile(r"periods: a trial pass \(no lengths stored\) took [0-9.]+ ms for \d+ suffixes, period (\d+)")


@pytest.mark.parametrize("q", sorted(lc.MULTIPLE_OF))
def test_stretches_in_a_list_above_the_dense_threshold(oracle, monkeypatch, capfd, q):
    """4 MiB with a 3 MiB stretch of period q: a list of more than 2^21 entries (the dense route).  The list the finder
    reads is in position order there, the winner is q itself and the division's trial passes -- q's prime factors, all in
    vain -- are tests/longperiodmodel.py divided()'s.  q = 4100 takes the long step; q = 1025 is the short finder's, and
    the switch changes nothing.  (A list in another order votes for a multiple of q: shown over a given list in
    tests/test_gpu_long_period_votes.py; no block was found whose own list does for a period above 4096.)"""
    d = lc.multiple_block(q)
    want = oracle.oracle_bwt_block(d, 8)
    left, tried = lm.divided(d, q)
    assert left == q and tried
    with _contexts(monkeypatch, d.size) as (ctx, ctx_off):
        if q > 4096:
            _stepped(ctx, ctx_off, d, q, 8, oracle, monkeypatch, capfd, ("dense", q))
        monkeypatch.setenv("BWTC_HIP_DEBUG", "1")
        capfd.readouterr()
        st = _same(ctx, d, 8, want, ("dense", q, "debug"))
        monkeypatch.delenv("BWTC_HIP_DEBUG")
        said = [int(x) for x in TRIAL_LINE.findall(capfd.readouterr().err)]
        print("q %d: trial passes %s, period %s, rounds %d route %#x" % (q, said, ctx.period(), st.rounds, st.route))
        assert said == tried, (said, tried)
        assert ctx.period()[0] == q and st.route & PERIOD_BIT and bool(st.route & LONG_BIT) == (q > 4096), (ctx.period(), hex(st.route))
        st_off = _same(ctx_off, d, 8, want, ("dense", q, "off"))
        if q > 4096:
            assert not st_off.route & (LONG_BIT | PERIOD_BIT) and ctx_off.period()[0] == 0 and st.rounds < st_off.rounds, (hex(st_off.route), st.rounds, st_off.rounds)
        else:
            assert (st.rounds, st.route, st.active_sum, st.alg_bytes) == (st_off.rounds, st_off.route, st_off.active_sum, st_off.alg_bytes) and ctx.period() == ctx_off.period()


def test_back_to_back_copies(oracle, monkeypatch, capfd):
    """64 KiB of text 32 times.  Under BWTC_HIP_COPIES=1 the waiting step keeps the copy gate shut: no pass, no copy round."""
    d = lc.back_to_back()
    with _contexts(monkeypatch, d.size) as (ctx, ctx_off):
        st, st_off = _stepped(ctx, ctx_off, d, 1 << 16, 8, oracle, monkeypatch, capfd, "back to back", zeros_off=False)
        assert st.rounds < st_off.rounds, (st.rounds, st_off.rounds)
    with _contexts(monkeypatch, d.size, "BWTC_HIP_COPIES=1") as (ctx, ctx_off):
        st, st_off = _stepped(ctx, ctx_off, d, 1 << 16, 8, oracle, monkeypatch, capfd, "back to back, copies", zeros_off=False)
        assert ctx.copies() == (0, 0, 0, 0) and not st.route & COPY_BIT, (ctx.copies(), hex(st.route))
        print("copies without the switch: %s, rounds %d" % (ctx_off.copies(), st_off.rounds))


def test_a_long_and_a_short_period(oracle, monkeypatch):
    """BWTC_HIP_MULTI=1: the stretches of period 9 and of period 5000 each take their step."""
    d = lc.long_and_short()
    want = oracle.oracle_bwt_block(d, 8)
    with _contexts(monkeypatch, 1 << 20, "BWTC_HIP_MULTI=1") as (ctx, ctx_off):
        st = _same(ctx, d, 8, want, "multi")
        ran = {e[0]: e[1] for e in ctx.schedule() if e[1]}
        print("schedule %s route %#x rounds %d" % (ctx.schedule(), st.route, st.rounds))
        assert set(ran) == {9, 5000} and 5000 <= ran[5000] < 10000, ctx.schedule()
        assert st.route & LONG_BIT and st.route & PERIOD_BIT and st.route & MULTI_BIT, hex(st.route)
        st_off = _same(ctx_off, d, 8, want, "multi, off")
        assert not st_off.route & LONG_BIT and {e[0] for e in ctx_off.schedule() if e[1]} == {9}, (hex(st_off.route), ctx_off.schedule())
        assert st.rounds < st_off.rounds, (st.rounds, st_off.rounds)


def test_forty_random_blocks(oracle, monkeypatch):
    """Every one of the 40 sets the bit with its own period (tests/test_longperiodmodel.py proves the premise)."""
    with _contexts(monkeypatch, 1 << 20) as (ctx, ctx_off):
        for it in range(40):
            d, p, L = lc.random_block(it)
            sp = (1, 8)[it % 2]
            want = oracle.oracle_bwt_block(d, sp)
            st = _same(ctx, d, sp, want, it)
            assert st.route & LONG_BIT and ctx.period()[0] == p and p <= ctx.period()[3] < 2 * p, (it, p, L, hex(st.route), ctx.period())
            st_off = _same(ctx_off, d, sp, want, (it, "off"))
            assert not st_off.route & LONG_BIT and ctx_off.period()[0] == 0 and st.rounds < st_off.rounds, (it, st.rounds, st_off.rounds, ctx_off.period())


def test_controls_are_untouched(oracle, monkeypatch):
    """Blocks of period 9 and 4096 and plain text: the same rounds, route, schedule and counted work with the switch and
    without it."""
    with _contexts(monkeypatch, 1 << 20) as (ctx, ctx_off), _contexts(monkeypatch, 1 << 20, "BWTC_HIP_MULTI=1") as (mctx, mctx_off):
        for what, d in lc.controls():
            want = oracle.oracle_bwt_block(d, 8)
            for on, off in ((ctx, ctx_off), (mctx, mctx_off)):
                a, b = _same(on, d, 8, want, what), _same(off, d, 8, want, (what, "off"))
                assert (a.rounds, a.route, a.active_sum, a.alg_bytes, a.sort_pass_items) == (b.rounds, b.route, b.active_sum, b.alg_bytes, b.sort_pass_items), what
                assert on.schedule() == off.schedule() and on.period() == off.period() and not a.route & LONG_BIT, what
