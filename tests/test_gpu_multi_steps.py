"""Closed-form steps for several periods in one block (BWTC_HIP_MULTI=1) on the GPU (-m gpu): every result -- bytes, LF
powers, freqs -- against oracle.oracle_bwt_block for 1 and 8 starting points, and Context.schedule(), the route
(bwtc_hip_stats.route bits 5, 8 and 9) and the rounds where the steps are the point.  A switch is read when a context is
made, so a test opens its own contexts.  The blocks are tests/multicases.py's; tests/test_multimodel.py proves their
premises, and tests/multimodel.py counts the rounds the rule takes.

The rounds' allowance is that of the period and mixed steps' tests, for the same three rounds: the text round behind
first-round steps, the round that confirms, and the depth at which the device's list stands when its rank[] is complete.
The model counts every step as a round of its own, so nothing is added per step.

Without the feature Context.schedule() does not exist and bit 9 is never set: a block with stretches of two periods takes
one period step and the other period's stretches double, log2(stretch / depth) rounds."""
import contextlib
import functools
import re

import numpy as np
import pytest

import mixedcases as mc
import multicases as cases
import multimodel as mu
import periodcases as pc

pytestmark = pytest.mark.gpu

RUN_BIT, PERIOD_BIT, SEVERAL_BIT = 32, 256, 512
SPS = (1, 8)
RUNS_LINE = re.compile(r"runs: longest run (\d+), the rounds begin at depth (\d+): (run step|no run step)")
STEPS_LINE = re.compile(r"steps: (\d+) entries((?:[:,] \(p \d+, depth \d+, gate \d+, votes \d+\))*)")


@contextlib.contextmanager
def _contexts(monkeypatch, size, extra="", others=("",)):
    """A context with BWTC_HIP_MULTI=1 and one per entry of `others` ("": no switch, else the switch's name), all with
    the switches of `extra`."""
    from bwtc_amd import hip
    names = []
    for one in extra.split(","):
        if one:
            name, value = one.split("=")
            monkeypatch.setenv(name, value)
            names.append(name)
    made = []
    try:
        for switch in ("BWTC_HIP_MULTI",) + tuple(others):
            if switch:
                monkeypatch.setenv(switch, "1")
            made.append(hip.Context(0, size))
            if switch:
                monkeypatch.delenv(switch)
        for name in names:
            monkeypatch.delenv(name)
        yield made
    finally:
        for c in made:
            c.close()


def _same(ctx, T, sp, want, what):
    got = ctx.bwt_block(cases.block(T), sp)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[2] == want[2]).all(), what
    return ctx.stats()


def _want(oracle, T, sp):
    return oracle.oracle_bwt_block(cases.block(T), sp)


def _said(ctx, T, sp, want, what, monkeypatch, capfd):
    """_same() with the sorter's debug lines: (stats, the depth the rounds begin at, the steps line's entries or None)."""
    monkeypatch.setenv("BWTC_HIP_DEBUG", "1")
    capfd.readouterr()
    try:
        st = _same(ctx, T, sp, want, what)
    finally:
        monkeypatch.delenv("BWTC_HIP_DEBUG")
    err = capfd.readouterr().err
    runs, steps = RUNS_LINE.findall(err), STEPS_LINE.findall(err)
    assert len(runs) == 1 and len(steps) <= 1, err[-2000:]
    line = [tuple(int(x) for x in e) for e in re.findall(r"\(p (\d+), depth (\d+), gate (\d+), votes (\d+)\)", steps[0][1])] if steps else None
    return st, int(runs[0][1]), line


def _ran(schedule):
    """The periods of the period steps that ran, in the schedule's order."""
    return [p for p, depth, _, _, _ in schedule if p >= 2 and depth]


def _consistent(st, schedule, what):
    """The schedule against the route bits and itself."""
    ran = [e for e in schedule if e[1]]
    periods = _ran(schedule)
    assert len(schedule) <= 4 and len([e for e in schedule if e[0] >= 2]) <= 3, (what, schedule)
    assert all(depth >= p for p, depth, _, _, _ in ran) and all(not (e[1] and e[4] & 2) for e in schedule), (what, schedule)
    assert [e[1] for e in ran] == sorted(e[1] for e in ran), (what, schedule)
    assert bool(st.route & PERIOD_BIT) == bool(periods) and bool(st.route & SEVERAL_BIT) == (len(periods) > 1), (what, hex(st.route), schedule)
    assert bool(st.route & RUN_BIT) == any(e[1] and (e[0] == 1 or e[4] & 1) for e in schedule), (what, hex(st.route), schedule)


@functools.lru_cache(maxsize=None)
def _model(key, periods, depth, merge=True):
    """The rounds and steps tests/multimodel.py takes over the block `key` names, with the run step and `periods`."""
    T = _block(key)
    _, rounds, steps = mu.sort_suffixes_np(T, (1,) + tuple(periods), depth, merge=merge)
    return rounds, steps


@functools.lru_cache(maxsize=None)
def _block(key):
    kind = key[0]
    if kind == "stretches":
        T = cases.stretches(key[1], key[2], run=key[3])
    elif kind == "merge":
        T = cases.merge_case()
    T.setflags(write=False)
    return T


def _steps_block(oracle, monkeypatch, capfd, ctx, ctx_off, key, periods, gap):
    """One block of planted periods on a context with the switch and one without: the bytes, the schedule against the model
    at the depth the device's rounds begin at, the rounds against the model's, and -- gap -- against the other context's."""
    T = _block(key)
    for sp in SPS:
        want = _want(oracle, T, sp)
        st, depth, line = _said(ctx, T, sp, want, (key, sp), monkeypatch, capfd)
        schedule = ctx.schedule()
        _consistent(st, schedule, (key, sp))
        model, model_steps = _model(key, periods, depth)
        print("%s sp %d: depth %d rounds %d route %#x schedule %s; model %d %s" % (key, sp, depth, st.rounds, st.route, schedule, model, model_steps))
        assert _ran(schedule) == [p for p, _ in model_steps if p >= 2], (key, sp, depth, schedule, model_steps)
        assert line == [e[:4] for e in schedule], (line, schedule)
        assert all(e[2] > 0 and (e[0] == 1 or e[3] >= max(256, T.size // 64)) for e in schedule), (key, schedule)
        assert ctx.period()[0] in periods and ctx.steps()[1] == _ran(schedule)[0], (ctx.period(), ctx.steps(), schedule)
        assert st.rounds <= model + 3, (key, sp, depth, st.rounds, model, model_steps)
        if ctx_off is not None:
            st_off = _same(ctx_off, T, sp, want, (key, sp, "off"))
            print("   without the switch: rounds %d route %#x period %s" % (st_off.rounds, st_off.route, ctx_off.period()))
            assert st_off.route & SEVERAL_BIT == 0 and len(_ran(ctx_off.schedule())) <= 1, (hex(st_off.route), ctx_off.schedule())
            if gap and key[2] >= 256 * max(max(periods), depth):
                assert st_off.rounds >= st.rounds + 6, (key, sp, st.rounds, st_off.rounds)
    return st, schedule


# ---- 1. two stretches in noise ---------------------------------------------------------------

@pytest.mark.parametrize("pair", cases.PAIRS)
def test_two_periods(oracle, monkeypatch, capfd, pair):
    """Stretches of two periods neither of which divides the other, 2^16 and 2^18 bytes, in noise: both steps run, in the
    model's order, within the model's rounds + 3; the context without the switch takes one period step and at least six
    rounds more where the stretches are 256 times max(p, depth) or longer."""
    with _contexts(monkeypatch, 1 << 20) as (ctx, ctx_off):
        for L in (1 << 16, 1 << 18):
            st, schedule = _steps_block(oracle, monkeypatch, capfd, ctx, ctx_off, ("stretches", pair, L, 0), pair, True)
            assert sorted(_ran(schedule)) == sorted(pair) and st.route & SEVERAL_BIT, (pair, L, schedule, hex(st.route))


def test_a_period_that_divides_the_other(oracle, monkeypatch, capfd):
    """Periods 3 and 6: a stretch of period 3 is one of period 6, so one of the two is skipped -- one period step, and the
    bytes are right."""
    with _contexts(monkeypatch, 1 << 20, others=()) as (ctx,):
        for L in (1 << 16, 1 << 18):
            T = cases.stretches(cases.DIVISOR_PAIR, L)
            for sp in SPS:
                st = _same(ctx, T, sp, _want(oracle, T, sp), (L, sp))
                _consistent(st, ctx.schedule(), (L, sp))
                assert len(_ran(ctx.schedule())) == 1 and _ran(ctx.schedule())[0] in cases.DIVISOR_PAIR, ctx.schedule()
                assert st.route & (PERIOD_BIT | SEVERAL_BIT) == PERIOD_BIT, hex(st.route)


@pytest.mark.parametrize("planted", sorted(cases.TRIPLES))
def test_three_periods(oracle, monkeypatch, capfd, planted):
    """Three stretches.  (5, 9, 64): three period steps.  (2, 9, 64): 64 is a multiple of 2, which has more votes, so the
    rule skips it -- two period steps, and the stretch of period 64 doubles."""
    takes = cases.TRIPLES[planted]
    with _contexts(monkeypatch, 1 << 20) as (ctx, ctx_off):
        st, schedule = _steps_block(oracle, monkeypatch, capfd, ctx, ctx_off, ("stretches", planted, 1 << 16, 0), takes, takes == planted)
        assert sorted(_ran(schedule)) == sorted(takes) and st.route & SEVERAL_BIT, (schedule, hex(st.route))


def test_a_run_beside_two_periods(oracle, monkeypatch, capfd):
    """A run of 2^16 zeros beside stretches of periods 9 and 300: the runs are ranked (bit 5), by the run step or by the
    first period step in its place, and both period steps run (bits 8 and 9)."""
    with _contexts(monkeypatch, 1 << 20) as (ctx, ctx_off):
        st, schedule = _steps_block(oracle, monkeypatch, capfd, ctx, ctx_off, ("stretches", (9, 300), 1 << 16, 1 << 16), (9, 300), False)
        assert st.route & (RUN_BIT | PERIOD_BIT | SEVERAL_BIT) == RUN_BIT | PERIOD_BIT | SEVERAL_BIT, (hex(st.route), schedule)
        gates = {e[0]: e[2] for e in schedule}
        # (the noise beside the run may go on with a zero)
        assert (1 << 16) <= gates.get(1, 1 << 16) <= (1 << 16) + 16 and all(abs(gates[p] - (1 << 16)) <= p for p in (9, 300)), schedule


# ---- 2. what the merge buys ------------------------------------------------------------------------

def test_the_merge_case(oracle, monkeypatch, capfd):
    """Three equal stretches per period behind equal tails.  Premise (tests/test_multimodel.py, and again here at the
    device's depth): the model's merged rounds are fewer than its overwrite rounds.  The device stays within merged + 3."""
    with _contexts(monkeypatch, 1 << 20, others=()) as (ctx,):
        T = _block(("merge",))
        for sp in SPS:
            st, depth, _ = _said(ctx, T, sp, _want(oracle, T, sp), ("merge", sp), monkeypatch, capfd)
            merged, steps = _model(("merge",), (9, 12), depth)
            over, _ = _model(("merge",), (9, 12), depth, False)
            print("merge case sp %d: depth %d rounds %d schedule %s; model merged %d overwrite %d" % (sp, depth, st.rounds, ctx.schedule(), merged, over))
            _consistent(st, ctx.schedule(), ("merge", sp))
            assert merged < over, (depth, merged, over)
            assert sorted(_ran(ctx.schedule())) == [9, 12] and st.rounds <= merged + 3, (depth, st.rounds, merged, ctx.schedule())


# ---- 3. seams -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", [(9, 12), (64, 300)])
def test_stretches_into_each_other_and_at_the_ends(oracle, monkeypatch, pair):
    """Stretches of two periods that run into each other and share bytes at the seam; falling and rising ends; a stretch
    that reaches the end of the text; a stretch that holds suffix 0."""
    with _contexts(monkeypatch, 1 << 20, others=()) as (ctx,):
        for what, T in cases.seam_blocks(*pair):
            for sp in SPS:
                st = _same(ctx, T, sp, _want(oracle, T, sp), (pair, what, sp))
                _consistent(st, ctx.schedule(), (pair, what, sp))
            print("%s %s: rounds %d route %#x schedule %s" % (pair, what, st.rounds, st.route, ctx.schedule()))
            assert sorted(_ran(ctx.schedule())) == sorted(pair), (pair, what, ctx.schedule())


# ---- 4. randomised --------------------------------------------------------------------------------------

def test_random_blocks(oracle, monkeypatch):
    """60 blocks, each with a stretch of 2^15 bytes or more for every one of two or three periods: the bytes, and several
    period steps in every one; every other block goes through the long-key route.  Two contexts, reused throughout."""
    with _contexts(monkeypatch, 1 << 20, others=()) as (ctx_plain,), \
            _contexts(monkeypatch, 1 << 20, "BWTC_HIP_GRAM_MIN_N=64", others=()) as (ctx_long,):
        for it in range(60):
            ctx = ctx_long if it % 2 else ctx_plain
            T, sp, periods = cases.random_block(it)
            st = _same(ctx, T, sp, _want(oracle, T, sp), (it, T.size, sp))
            _consistent(st, ctx.schedule(), it)
            assert len(_ran(ctx.schedule())) >= 2 and set(_ran(ctx.schedule())) <= set(periods), (it, periods, T.size, hex(st.route), ctx.schedule())


# ---- 5. reuse ----------------------------------------------------------------------------------------------

def test_one_context_large_tiny_large(oracle, monkeypatch):
    with _contexts(monkeypatch, 1 << 20, others=()) as (ctx,):
        large = cases.stretches((9, 300), 1 << 17)
        tiny = np.array([5, 5, 6, 5, 5, 6, 5], np.uint8)
        plain = np.random.default_rng(8).integers(0, 256, 200000).astype(np.uint8)
        for what, T in (("large", large), ("tiny", tiny), ("large", cases.block(large)), ("plain", plain), ("large", large)):
            sp = 8 if T.size > 100 else 1
            st = _same(ctx, T, sp, _want(oracle, T, sp), what)
            _consistent(st, ctx.schedule(), what)
            if what == "large":
                assert sorted(_ran(ctx.schedule())) == [9, 300] and st.route & SEVERAL_BIT, (hex(st.route), ctx.schedule())
            else:
                assert ctx.schedule() == [] and st.route & (PERIOD_BIT | SEVERAL_BIT) == 0, (what, hex(st.route), ctx.schedule())


# ---- 6. one period or none: MIXED's block -------------------------------------------------------------------

def test_one_period_or_none_is_what_mixed_does(oracle, monkeypatch):
    """Blocks with one period, with a run and one period, and with nothing of the kind: a context with BWTC_HIP_MULTI=1
    and one with BWTC_HIP_MIXED=1 take the same rounds, route and steps(), and no block shows bit 9."""
    blocks = [(what, cases.block(d)) for what, d in mc.plain_blocks()]
    blocks += [("a run and a stretch of period %d" % p, cases.block(mc.run_and_stretch(p, 1 << 16, 1 << 16))) for p in (2, 9, 64, 300)]
    blocks += [("one stretch of period %d" % p, cases.stretches((p,), 1 << 16)) for p in (9, 300)]
    with _contexts(monkeypatch, 1 << 20, others=("BWTC_HIP_MIXED",)) as (ctx, ctx_mixed):
        for what, T in blocks:
            want = _want(oracle, T, 8)
            st = _same(ctx, T, 8, want, what)
            st_mixed = _same(ctx_mixed, T, 8, want, (what, "mixed"))
            print("%s: rounds %d route %#x steps %s schedule %s against rounds %d route %#x" % (what, st.rounds, st.route, ctx.steps(), ctx.schedule(), st_mixed.rounds, st_mixed.route))
            assert (st.rounds, st.route, ctx.steps()) == (st_mixed.rounds, st_mixed.route, ctx_mixed.steps()), (what, st.rounds, st_mixed.rounds, hex(st.route), hex(st_mixed.route), ctx.steps(), ctx_mixed.steps())
            assert st.route & SEVERAL_BIT == 0, (what, hex(st.route))
            _consistent(st, ctx.schedule(), what)
