"""The run step AND a period step in one block (BWTC_HIP_MIXED=1) on the GPU (-m gpu): every result -- bytes, LF powers,
freqs -- against oracle.oracle_bwt_block for 1 and 8 starting points, and the route (bwtc_hip_stats.route bits 5 and 8),
bwtc_hip_steps_get and the rounds where the two steps are the point.  A switch is read when a context is made, so a test
opens its own pair: one with BWTC_HIP_MIXED=1 and one without.  The blocks are tests/mixedcases.py's;
tests/test_mixedmodel.py proves their premises, and tests/mixedmodel.py counts the rounds the rule takes.

Without the feature Context.steps() does not exist and bit 8 is never set beside bit 5: a block with a long run takes the
run step alone and its stretches double, log2(stretch / depth) rounds."""
import contextlib
import functools
import re

import numpy as np
import pytest

import mixedcases as mc
import mixedmodel
import periodcases as pc

pytestmark = pytest.mark.gpu

RUN_BIT, PERIOD_BIT = 32, 256
BOTH = RUN_BIT | PERIOD_BIT
SPS = (1, 8)
RUNS_LINE = re.compile(r"runs: longest run (\d+), the rounds begin at depth (\d+): (run step|no run step)")
STEPS_LINE = re.compile(r"steps: run step at depth (\d+), period step of period (\d+) at depth (\d+), longest run (\d+), longest proper stretch (\d+)")


@contextlib.contextmanager
def _contexts(monkeypatch, size, extra="", off=True):
    """(context with BWTC_HIP_MIXED=1, context without it or None), both with the switches of `extra`."""
    from bwtc_amd import hip
    names = []
    for one in extra.split(","):
        if one:
            name, value = one.split("=")
            monkeypatch.setenv(name, value)
            names.append(name)
    monkeypatch.setenv("BWTC_HIP_MIXED", "1")
    ctx_on = hip.Context(0, size)
    monkeypatch.delenv("BWTC_HIP_MIXED")
    ctx_off = hip.Context(0, size) if off else None
    for name in names:
        monkeypatch.delenv(name)
    try:
        yield ctx_on, ctx_off
    finally:
        ctx_on.close()
        if ctx_off is not None:
            ctx_off.close()


def _same(ctx, d, sp, want, what):
    got = ctx.bwt_block(d, sp)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[2] == want[2]).all(), what
    return ctx.stats()


def _said(ctx, d, sp, want, what, monkeypatch, capfd):
    """_same() with the sorter's debug lines: (stats, the depth the rounds begin at, the steps line's numbers or None)."""
    monkeypatch.setenv("BWTC_HIP_DEBUG", "1")
    capfd.readouterr()
    try:
        st = _same(ctx, d, sp, want, what)
    finally:
        monkeypatch.delenv("BWTC_HIP_DEBUG")
    err = capfd.readouterr().err
    runs, steps = RUNS_LINE.findall(err), STEPS_LINE.findall(err)
    assert len(runs) == 1 and len(steps) <= 1, err[-2000:]
    return st, int(runs[0][1]), tuple(int(x) for x in steps[0]) if steps else None


@functools.lru_cache(maxsize=None)
def _model_rounds(p, run, stretch, depth):
    """The rounds tests/mixedmodel.py takes over the block as the sorter sees it (reversed), and its steps."""
    d = mc.run_and_stretch(p, run, stretch)
    _, rounds, steps = mixedmodel.sort_suffixes_np(d[::-1].copy(), p, depth)
    return rounds, steps


# ---- 1. a run and a stretch ---------------------------------------------------------------

@pytest.mark.parametrize("p", [2, 9, 64, 300])
def test_a_run_and_a_stretch(oracle, monkeypatch, capfd, p):
    """A zero run and a stretch of a primitive unit of period p, 2^16 and 2^18 bytes each way, in noise.  With the switch:
    both bits, steps() names p and both depths, and the rounds are at most the model's for that block and depth plus 3 --
    the allowance of the period step's own tests (ceil(log2(p / d)) + 3 there): the text round behind a first-round step,
    the round that confirms, and one for the depth at which the device's list stands when its rank[] is complete.
    Without it the block takes the run step alone, and at least six rounds more where the stretch is 256 times
    max(p, d) or longer.  On the sorter without the feature steps() does not exist and bit 8 stays clear."""
    with _contexts(monkeypatch, 1 << 20) as (ctx, ctx_off):
        for run, stretch in ((1 << 16, 1 << 16), (1 << 18, 1 << 16), (1 << 16, 1 << 18)):
            d = mc.run_and_stretch(p, run, stretch)
            for sp in SPS:
                want = oracle.oracle_bwt_block(d, sp)
                st, depth, line = _said(ctx, d, sp, want, (p, run, stretch, sp), monkeypatch, capfd)
                st_off = _same(ctx_off, d, sp, want, (p, run, stretch, sp, "off"))
                run_depth, got_p, period_depth, longest_run, proper = ctx.steps()
                model, model_steps = _model_rounds(p, run, stretch, depth)
                print("p %d run %d stretch %d sp %d: depth %d rounds %d route %#x steps %s; model %d %s; off: rounds %d route %#x"
                      % (p, run, stretch, sp, depth, st.rounds, st.route, ctx.steps(), model, model_steps, st_off.rounds, st_off.route))
                assert st.route & BOTH == BOTH, (p, run, stretch, sp, hex(st.route), ctx.steps())
                assert st_off.route & BOTH == RUN_BIT and ctx_off.steps()[1:3] == (0, 0), (hex(st_off.route), ctx_off.steps())
                assert got_p == p and run_depth >= depth and period_depth >= max(p, run_depth), (p, depth, ctx.steps())
                assert (period_depth == run_depth) == (p <= depth), (p, depth, ctx.steps())
                assert longest_run == run and stretch - p <= proper <= stretch + p, (p, run, stretch, ctx.steps())
                assert line == (run_depth, p, period_depth, run, proper), (line, ctx.steps())
                assert ctx.period()[0] == p and ctx.period()[3] == period_depth, ctx.period()
                assert [q for q, _ in model_steps] == ([p] if p <= depth else [1, p]), (p, depth, model_steps)
                assert st.rounds <= model + 3, (p, run, stretch, sp, st.rounds, model)
                if stretch >= 256 * max(p, depth):
                    assert st_off.rounds >= st.rounds + 6, (p, run, stretch, sp, st.rounds, st_off.rounds)


# ---- 2. the members whose k_1 is dropped ---------------------------------------------------

@pytest.mark.parametrize("p", [64, 300])
def test_short_runs_beside_stretches(oracle, monkeypatch, capfd, p):
    """Runs of 16 ... p - 1 bytes beside stretches of period p, and a stretch of a unit a...ab with an inner run that long:
    the run step ranks them by k_1, and the period step's lengths take k_1's place.  Premise, from the debug line: the
    rounds begin at a depth of 16 at the most."""
    d = mc.short_runs_beside_stretches(p, 16)
    with _contexts(monkeypatch, 1 << 20, off=False) as (ctx, _):
        for sp in SPS:
            st, depth, line = _said(ctx, d, sp, oracle.oracle_bwt_block(d, sp), (p, sp), monkeypatch, capfd)
            print("p %d sp %d: depth %d rounds %d route %#x steps %s" % (p, sp, depth, st.rounds, st.route, ctx.steps()))
            assert depth <= 16 < p, depth
            assert st.route & BOTH == BOTH and ctx.steps()[1] == p and ctx.steps()[0] < p <= ctx.steps()[2], (hex(st.route), ctx.steps())


# ---- 3. runs and stretches that run into each other ------------------------------------------

@pytest.mark.parametrize("p", [3, 9, 64])
def test_runs_into_stretches_and_back(oracle, monkeypatch, p):
    """A run that ends where a stretch begins with the run's byte, and a stretch that ends in a run; falling and rising."""
    stepped = 0
    blocks = mc.seam_blocks(p)
    with _contexts(monkeypatch, 1 << 20, off=False) as (ctx, _):
        for what, d in blocks:
            for sp in SPS:
                st = _same(ctx, d, sp, oracle.oracle_bwt_block(d, sp), (p, what, sp))
            print("p %d %s: rounds %d route %#x steps %s period %s" % (p, what, st.rounds, st.route, ctx.steps(), ctx.period()))
            stepped += st.route & BOTH == BOTH
    assert stepped == len(blocks), (stepped, len(blocks))


# ---- 4. nothing mixed -------------------------------------------------------------------------

def test_nothing_mixed_nothing_changes(oracle, monkeypatch):
    """Zeros, one run in noise, one stretch without runs, random bytes, the generator's text: no bit that the context
    without the switch does not set, the same rounds and active_sum, equal bytes."""
    with _contexts(monkeypatch, 1 << 20) as (ctx, ctx_off):
        for what, d in mc.plain_blocks():
            want = oracle.oracle_bwt_block(d, 8)
            st = _same(ctx, d, 8, want, what)
            st_off = _same(ctx_off, d, 8, want, (what, "off"))
            print("%s: rounds %d route %#x steps %s against rounds %d route %#x" % (what, st.rounds, st.route, ctx.steps(), st_off.rounds, st_off.route))
            assert st.route & ~st_off.route == 0 and st.route & BOTH != BOTH, (what, hex(st.route), hex(st_off.route))
            assert st.rounds == st_off.rounds and st.active_sum == st_off.active_sum, (what, st.rounds, st_off.rounds, st.active_sum, st_off.active_sum)


# ---- 5. routes ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _big_block():
    d = np.random.default_rng(12).integers(0, 256, 4 << 20).astype(np.uint8)
    d[1 << 19:(1 << 19) + (1 << 20)] = 0
    d[2 << 20:3 << 20] = pc.stretch(9, 1 << 20)
    d.setflags(write=False)
    import oracle_lib
    return d, oracle_lib.oracle_bwt_block(d, 8)


@pytest.mark.parametrize("extra", ["", "BWTC_HIP_GRAM_MIN_N=64", "BWTC_HIP_LONG=0"])
def test_a_run_and_a_stretch_at_4MiB(oracle, monkeypatch, extra):
    """Random bytes with a 1 MiB zero run and a 1 MiB stretch of period 9: the long-key route and, with a list far above
    the dense route's threshold, the dense route.  Both bits."""
    d, want = _big_block()
    with _contexts(monkeypatch, d.size, extra) as (ctx, ctx_off):
        st = _same(ctx, d, 8, want, extra)
        st_off = _same(ctx_off, d, 8, want, (extra, "off"))
        print("%s: rounds %d (route %#x, steps %s) against %d (route %#x)" % (extra, st.rounds, st.route, ctx.steps(), st_off.rounds, st_off.route))
        assert st.route & BOTH == BOTH and ctx.steps()[1] == 9, (hex(st.route), ctx.steps())
        assert st_off.route & BOTH == RUN_BIT, hex(st_off.route)


@pytest.mark.parametrize("extra", ["BWTC_HIP_GRAM_MIN_N=64", "BWTC_HIP_GRAM_MIN_N=64,BWTC_HIP_FINISHER=0", "BWTC_HIP_DENSE=0"])
def test_the_long_key_route_below_1MiB(oracle, monkeypatch, extra):
    with _contexts(monkeypatch, 1 << 20, extra, off=False) as (ctx, _):
        for p in (9, 64):
            d = mc.run_and_stretch(p, 1 << 16, 1 << 17)
            for sp in SPS:
                st = _same(ctx, d, sp, oracle.oracle_bwt_block(d, sp), (extra, p, sp))
                print("%s p %d sp %d: rounds %d route %#x steps %s" % (extra, p, sp, st.rounds, st.route, ctx.steps()))
                assert st.route & BOTH == BOTH and ctx.steps()[1] == p, (extra, p, hex(st.route), ctx.steps())


# ---- 6. forced periods ---------------------------------------------------------------------------

@pytest.mark.parametrize("forced", ["true", "double", "wrong"])
def test_forced_periods(oracle, monkeypatch, forced):
    """BWTC_HIP_PERIOD = the true p, 2 p and a wrong p with the switch: the bytes are right whatever the period; the true
    p takes both steps."""
    for p in (3, 64):
        value = {"true": p, "double": 2 * p, "wrong": p + 2}[forced]
        with _contexts(monkeypatch, 1 << 20, "BWTC_HIP_PERIOD=%d" % value, off=False) as (ctx, _):
            blocks = [("a run and a stretch", mc.run_and_stretch(p, 1 << 16, 1 << 16))] + mc.seam_blocks(p)[:2] + pc.tie_blocks(p, 3000)[:2]
            for what, d in blocks:
                for sp in SPS:
                    st = _same(ctx, d, sp, oracle.oracle_bwt_block(d, sp), (forced, p, what, sp))
                if what == "a run and a stretch" and forced == "true":
                    assert st.route & BOTH == BOTH and ctx.steps()[1] == p, (p, hex(st.route), ctx.steps())


# ---- 7. reuse --------------------------------------------------------------------------------------

def test_one_context_mixed_plain_mixed_tiny(oracle, monkeypatch):
    with _contexts(monkeypatch, 1 << 20, off=False) as (ctx, _):
        mixed = mc.run_and_stretch(64, 1 << 16, 1 << 16)
        plain = np.random.default_rng(8).integers(0, 256, 200000).astype(np.uint8)
        tiny = np.array([5, 5, 6, 5, 5, 6, 5], np.uint8)
        for what, d in (("mixed", mixed), ("plain", plain), ("mixed", mixed[::-1].copy()), ("tiny", tiny), ("mixed", mixed)):
            st = _same(ctx, d, 8 if d.size > 100 else 1, oracle.oracle_bwt_block(d, 8 if d.size > 100 else 1), what)
            run_depth, p, period_depth, _, proper = ctx.steps()
            if what == "mixed":
                assert st.route & BOTH == BOTH and p == 64 and 0 < run_depth < 64 <= period_depth, (hex(st.route), ctx.steps())
            else:
                assert st.route & BOTH == 0 and (run_depth, p, period_depth, proper) == (0, 0, 0, 0), (what, hex(st.route), ctx.steps())


# ---- 8. randomised -----------------------------------------------------------------------------------

def test_random_mixed_blocks(oracle, monkeypatch):
    """60 blocks, each with a run of 4096 bytes or more and a voted stretch of 2^15 or more: every one shows both bits;
    every other block goes through the long-key route.  Two contexts with the switch, reused throughout."""
    with _contexts(monkeypatch, 1 << 20, off=False) as (ctx_plain, _), \
            _contexts(monkeypatch, 1 << 20, "BWTC_HIP_GRAM_MIN_N=64", off=False) as (ctx_long, _):
        for it in range(60):
            ctx = ctx_long if it % 2 else ctx_plain
            d, sp, p = mc.random_block(it)
            st = _same(ctx, d, sp, oracle.oracle_bwt_block(d, sp), (it, d.size, sp))
            assert st.route & BOTH == BOTH and ctx.steps()[1] == p, (it, p, d.size, hex(st.route), ctx.steps(), ctx.period())


# ---- 9. the schedule beside steps() and period(), with no switch, MIXED and MULTI -------------------

def test_the_schedule_agrees_with_steps_and_period(oracle, monkeypatch):
    """One stretch (first round's and deferred) and a run beside one (merged into one step, and the step behind the run
    step) on a context with no switch, one with BWTC_HIP_MIXED=1 and one with BWTC_HIP_MULTI=1: the bytes; schedule()'s
    periods and depths are steps()'s and period()'s; gate and votes are 0 without MULTI, and with it a period entry's
    gate is the longest proper stretch and the run entry's the longest run."""
    from bwtc_amd import hip
    blocks = [("stretch 9", pc.stretch(9, 1 << 16)), ("stretch 257", pc.stretch(257, 1 << 16)),
              ("run and stretch 9", mc.run_and_stretch(9, 1 << 16, 1 << 16)), ("run and stretch 300", mc.run_and_stretch(300, 1 << 16, 1 << 16)),
              # (the four above have one length for the longest run, stretch and proper stretch; this one has three)
              ("short runs beside stretches", mc.short_runs_beside_stretches(64, 16))]
    wants = [oracle.oracle_bwt_block(d, 8) for _, d in blocks]
    stepped = set()
    for switch in ("", "BWTC_HIP_MIXED", "BWTC_HIP_MULTI"):
        if switch:
            monkeypatch.setenv(switch, "1")
        ctx = hip.Context(0, 1 << 20)
        if switch:
            monkeypatch.delenv(switch)
        with ctx:
            for (what, d), want in zip(blocks, wants):
                _same(ctx, d, 8, want, (switch, what))
                schedule, steps, period = ctx.schedule(), ctx.steps(), ctx.period()
                print("%s [%s]: schedule %s steps %s period %s" % (what, switch, schedule, steps, period))
                runs = [e for e in schedule if e[0] == 1 or e[4] & 1]
                periods = [e for e in schedule if e[0] >= 2]
                ran = [e for e in periods if e[1]]
                assert len(runs) <= 1 and len(periods) <= 1, (switch, what, schedule)
                assert steps[0] == (runs[0][1] if runs else 0), (switch, what, schedule, steps)
                assert (steps[1], steps[2]) == (ran[0][:2] if ran else (0, 0)) and period[3] == steps[2], (switch, what, schedule, steps, period)
                assert all(e[0] == period[0] for e in periods), (switch, what, schedule, period)
                if switch == "BWTC_HIP_MULTI":
                    assert all(e[2] == steps[4] for e in periods), (what, schedule, steps)
                    assert all(e[2] == steps[3] for e in schedule if e[0] == 1), (what, schedule, steps)
                else:
                    assert all(e[2] == 0 and e[3] == 0 for e in schedule), (switch, what, schedule)
                if ran:
                    stepped.add((switch, what))
    # (every block takes its period step on some context, so the words compared above are not all zeros)
    assert {what for _, what in stepped} == {what for what, _ in blocks}, stepped
