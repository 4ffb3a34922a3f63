"""Copy rounds (BWTC_HIP_COPIES=1) on the GPU (-m gpu): every result -- bytes, LF powers, freqs -- against
oracle.oracle_bwt_block for 1 and 8 starting points, and Context.copies(), the route (bwtc_hip_stats.route bit 10) and the
rounds where the copies are the point.  A switch is read when a context is made, so a test opens its own contexts.  The
blocks are tests/copycases.py's; tests/test_copymodel.py proves their premises, and tests/copymodel.py counts the rounds
the rule takes.

The rounds' allowance is that of the period and mixed steps' tests, three rounds: a text round before rank[] is complete,
the round that confirms, and the depth at which the device's list stands when its rank[] is complete.

Without the feature Context.copies() does not exist and bit 10 is never set."""
import contextlib
import functools
import re

import numpy as np
import pytest

import copycases as cases
import copymodel as cm

pytestmark = pytest.mark.gpu

COPY_BIT, RUN_BIT, PERIOD_BIT = 1024, 32, 256
SPS = (1, 8)
COPIES_LINE = re.compile(r"copies: (\d+) passes, (\d+) copy rounds, longest K (\d+), first depth (\d+), the rounds begin at depth (\d+)")
EXTRAS = ("", "BWTC_HIP_TEXT_ROUNDS=0", "BWTC_HIP_FINISHER=0", "BWTC_HIP_LONG=0", "BWTC_HIP_KEYS=grams", "BWTC_HIP_DENSE=0", "BWTC_HIP_RUNS=0",
          "BWTC_HIP_PERIODS=0", "BWTC_HIP_MIXED=1", "BWTC_HIP_MULTI=1")


@contextlib.contextmanager
def _contexts(monkeypatch, size, extra="", others=("",)):
    """A context with BWTC_HIP_COPIES=1 and one per entry of `others` ("": no switch), all with the switches of `extra`."""
    from bwtc_amd import hip
    names = []
    for one in extra.split(","):
        if one:
            name, value = one.split("=")
            monkeypatch.setenv(name, value)
            names.append(name)
    made = []
    try:
        for switch in ("BWTC_HIP_COPIES",) + tuple(others):
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


@functools.lru_cache(maxsize=None)
def _copy_blocks():
    out = cases.copy_blocks()
    for _, T, _, _ in out:
        T.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(oracle, which, sp):
    """The oracle's answer for copy block `which`, made once."""
    return oracle.oracle_bwt_block(cases.block(_copy_blocks()[which][1]), sp)


@functools.lru_cache(maxsize=None)
def _model(which, depth):
    return cm.sort_suffixes_np(_copy_blocks()[which][1], depth)[1]


def _same(ctx, T, sp, want, what):
    got = ctx.bwt_block(cases.block(T), sp)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[2] == want[2]).all(), what
    return ctx.stats()


def _said(ctx, T, sp, want, what, monkeypatch, capfd):
    """_same() with the sorter's debug lines: (stats, the last `copies:` line's numbers)."""
    monkeypatch.setenv("BWTC_HIP_DEBUG", "1")
    capfd.readouterr()
    try:
        st = _same(ctx, T, sp, want, what)
    finally:
        monkeypatch.delenv("BWTC_HIP_DEBUG")
    lines = COPIES_LINE.findall(capfd.readouterr().err)
    assert lines, what
    return st, tuple(int(x) for x in lines[-1])


@pytest.mark.parametrize("extra", EXTRAS)
def test_copies_behind_fillers_shuffled_and_with_inner_repeats(oracle, monkeypatch, capfd, extra):
    """2, 12 and 300 copies of a piece of letters behind fillers of 1 ... 300 bytes, a piece of words, two pieces shuffled:
    the bytes; bit 10 and copies(); the rounds within the model's from the depth the device's rounds begin at, plus 3; and
    fewer rounds than the context without the switch takes."""
    extra = extra + ",BWTC_HIP_GRAM_MIN_N=64" if extra in ("", "BWTC_HIP_TEXT_ROUNDS=0", "BWTC_HIP_KEYS=grams") else extra
    with _contexts(monkeypatch, 1 << 20, extra) as (ctx, ctx_off):
        for which, (name, T, _, _) in enumerate(_copy_blocks()):
            for sp in SPS:
                want = _want(oracle, which, sp)
                st, (passes, rounds, longest, first, begin) = _said(ctx, T, sp, want, (extra, name, sp), monkeypatch, capfd)
                model = _model(which, begin)
                st_off = _same(ctx_off, T, sp, want, (extra, name, sp, "off"))
                print("%s [%s] sp %d: rounds %d route %#x copies %s, the rounds begin at %d: model %d; without the switch %d rounds, route %#x"
                      % (name, extra, sp, st.rounds, st.route, ctx.copies(), begin, model, st_off.rounds, st_off.route))
                assert st.route & COPY_BIT and ctx.copies() == (rounds, passes, longest, first), (name, hex(st.route), ctx.copies())
                assert 1 <= rounds <= passes <= rounds + 1 and first >= begin and longest >= 1, (name, ctx.copies())
                assert st.rounds <= model + 3, (extra, name, sp, begin, st.rounds, model)
                assert st_off.route & COPY_BIT == 0 and st_off.rounds > st.rounds, (extra, name, sp, st.rounds, st_off.rounds)
                assert ctx_off.copies() == (0, 0, 0, 0)


def test_blocks_without_copies(oracle, monkeypatch):
    """Random bytes, letters, four symbols: the same rounds and route with the switch and without, bit 10 clear."""
    with _contexts(monkeypatch, 1 << 20) as (ctx, ctx_off):
        for name, T in cases.plain_blocks():
            want = oracle.oracle_bwt_block(cases.block(T), 8)
            st, st_off = _same(ctx, T, 8, want, name), _same(ctx_off, T, 8, want, (name, "off"))
            print("%s: rounds %d route %#x copies %s against rounds %d route %#x" % (name, st.rounds, st.route, ctx.copies(), st_off.rounds, st_off.route))
            assert (st.rounds, st.route) == (st_off.rounds, st_off.route) and st.route & COPY_BIT == 0, (name, st.rounds, st_off.rounds, hex(st.route))
            assert ctx.copies()[0] == 0


def test_a_step_and_copies(oracle, monkeypatch):
    """Copies beside a long run or a long stretch of period 9: the closed-form step runs, no copy round, right bytes."""
    with _contexts(monkeypatch, 1 << 20, others=()) as (ctx,):
        for name, T, bit in cases.step_blocks():
            for sp in SPS:
                st = _same(ctx, T, sp, oracle.oracle_bwt_block(cases.block(T), sp), (name, sp))
                print("%s sp %d: rounds %d route %#x copies %s steps %s" % (name, sp, st.rounds, st.route, ctx.copies(), ctx.steps()))
                assert st.route & bit and st.route & COPY_BIT == 0 and ctx.copies() == (0, 0, 0, 0), (name, hex(st.route), ctx.copies())


def test_random_blocks(oracle, monkeypatch):
    """100 copy-structured blocks of at most 64 KiB on one pair of contexts (every other block through the long-key
    route): the bytes, and bit 10 exactly where copies() counts a round."""
    with _contexts(monkeypatch, 1 << 16, others=()) as (ctx_plain,), \
            _contexts(monkeypatch, 1 << 16, "BWTC_HIP_GRAM_MIN_N=64", others=()) as (ctx_long,):
        ran = 0
        for it in range(100):
            ctx = ctx_long if it % 2 else ctx_plain
            T, sp = cases.random_block(it)
            st = _same(ctx, T, sp, oracle.oracle_bwt_block(cases.block(T), sp), (it, T.size, sp))
            rounds, passes, longest, first = ctx.copies()
            assert bool(st.route & COPY_BIT) == (rounds > 0) and rounds <= passes and (longest > 0) == (rounds > 0), (it, hex(st.route), ctx.copies())
            ran += rounds > 0
        print("%d of 100 blocks took a copy round" % ran)
        assert ran >= 25                                    # (a quarter of them: enough for the case to be about copy rounds)


def test_one_context_copies_plain_copies(oracle, monkeypatch):
    with _contexts(monkeypatch, 1 << 20, others=()) as (ctx,):
        name, T, _, _ = _copy_blocks()[1]
        plain = np.random.default_rng(8).integers(0, 256, 200000).astype(np.uint8)
        tiny = np.array([5, 5, 6, 5, 5, 6, 5], np.uint8)
        for what, X, which in (("copies", T, 1), ("plain", plain, None), ("tiny", tiny, None), ("copies", T, 1)):
            sp = 8 if X.size > 100 else 1
            want = _want(oracle, which, sp) if which is not None else oracle.oracle_bwt_block(cases.block(X), sp)
            st = _same(ctx, X, sp, want, what)
            if what == "copies":
                assert st.route & COPY_BIT and ctx.copies()[0] >= 1 and ctx.copies()[2] >= 1 << 13, (hex(st.route), ctx.copies())
            else:
                assert st.route & COPY_BIT == 0 and ctx.copies()[0] == 0, (what, hex(st.route), ctx.copies())
