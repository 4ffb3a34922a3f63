"""The suffix sorter's period step on the GPU (-m gpu): blocks with stretches of a period p > 1, every result -- bytes,
LF powers, freqs -- against oracle.oracle_bwt_block, and the rounds, the route (bwtc_hip_stats.route bit 8) and
bwtc_hip_period_get where the step is the point.  A switch is read when a context is made, so every test opens its own
contexts: one as shipped and, where rounds are compared, one with BWTC_HIP_PERIODS=0 (the sorter without the votes, the
pass and the step).  The blocks are tests/periodcases.py's; tests/test_periodmodel.py proves their premises.

Without the period step the getter does not exist and the asserts on `route & 256` and on the rounds of cases 1, 3 and
5 fail: a stretch of L bytes then takes log2(L / depth) doubling rounds."""
import contextlib
import functools
import math
import re

import numpy as np
import pytest

import periodcases as pc
from bwtc_amd import synth

pytestmark = pytest.mark.gpu

RUN_BIT, PERIOD_BIT = 32, 256
SPS = (1, 8, 256)
DEBUG_LINE = re.compile(r"periods: period (\d+) with (\d+) votes, longest stretch (\d+), the rounds begin at depth (\d+): "
                        r"(period step at depth (\d+)|no period step)")
RUNS_LINE = re.compile(r"runs: longest run (\d+), the rounds begin at depth (\d+): (run step|no run step)")


@contextlib.contextmanager
def _contexts(monkeypatch, size, extra="", off=True):
    """(context as shipped, context with BWTC_HIP_PERIODS=0 or None), both with the switches of `extra`."""
    from bwtc_amd import hip
    names = []
    for one in extra.split(","):
        if one:
            name, value = one.split("=")
            monkeypatch.setenv(name, value)
            names.append(name)
    monkeypatch.delenv("BWTC_HIP_PERIODS", raising=False)
    ctx_on = hip.Context(0, size)
    ctx_off = None
    if off:
        monkeypatch.setenv("BWTC_HIP_PERIODS", "0")
        ctx_off = hip.Context(0, size)
        monkeypatch.delenv("BWTC_HIP_PERIODS")
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


def _said(ctx, d, sp, want, what, monkeypatch, capfd, runs_on=True):
    """_same() with the sorter's debug lines: (stats, the periods line's fields or None, every runs line)."""
    monkeypatch.setenv("BWTC_HIP_DEBUG", "1")
    capfd.readouterr()
    try:
        st = _same(ctx, d, sp, want, what)
    finally:
        monkeypatch.delenv("BWTC_HIP_DEBUG")
    err = capfd.readouterr().err
    lines = DEBUG_LINE.findall(err)
    assert len(lines) <= 1, lines
    # the runs' line: exactly once per block that reaches the doubling rounds with the run ranking on (a block that looks
    # for a period is one), never twice
    assert len(RUNS_LINE.findall(err)) == (1 if lines and runs_on else min(1, len(RUNS_LINE.findall(err)))), err[-2000:]
    line = None
    if lines:
        p, votes, longest, depth, said, at = lines[0]
        line = dict(p=int(p), votes=int(votes), longest=int(longest), depth=int(depth), stepped=said != "no period step",
                    at=int(at) if at else 0, passes=len(re.findall(r"periods: the period-length pass took", err)))
    return st, line, RUNS_LINE.findall(err)


def _words(n, sigma, seed, lowest=1):
    """Random words over sigma symbols (none below `lowest`), n bytes."""
    rng = np.random.default_rng(seed)
    alphabet = rng.choice(np.arange(lowest, 256), sigma, replace=False).astype(np.uint8)
    words = [alphabet[rng.integers(0, sigma, int(rng.integers(1, 9)))] for _ in range(150)]
    return np.concatenate([words[int(i)] for i in rng.integers(0, len(words), n // 3 + 8)])[:n].copy()


# ---- 1. one stretch -----------------------------------------------------------------------

@pytest.mark.parametrize("p", [2, 3, 9, 64, 257, 4096])
def test_one_stretch(oracle, monkeypatch, capfd, p):
    """A unit of p random bytes (primitive: its last byte occurs once) repeated to 2^12, 2^14, 2^16, 2^18 and 2^20 + 3
    bytes.  From 2^16 bytes up the step must have run with that p and the rounds stay within
    ceil(log2(max(1, p / d))) + 3 -- d the depth the rounds begin at, from the sorter's debug line.  The sorter without
    the step takes at least six rounds more: asserted where the stretch is at least 256 times max(p, d) long.  Below
    that the premise cannot hold -- the plain sorter is through after about log2(n / d) + 1 rounds, the step's after
    log2(p / d) + 2, and 2^16 bytes are sixteen periods of 4096: four doublings -- so there the difference is printed."""
    sizes = [1 << 12, 1 << 14, 1 << 16, 1 << 18, (1 << 20) + 3]
    with _contexts(monkeypatch, (1 << 20) + 3) as (ctx, ctx_off):
        for n in sizes:
            d = pc.stretch(p, n)
            for sp in SPS:
                want = oracle.oracle_bwt_block(d, sp)
                st, line, _ = _said(ctx, d, sp, want, (p, n, sp), monkeypatch, capfd)
                st_off = _same(ctx_off, d, sp, want, (p, n, sp, "off"))
                print("p %d, %d bytes, %d starting points: rounds %d route %#x (%s) against %d route %#x"
                      % (p, n, sp, st.rounds, st.route, line, st_off.rounds, st_off.route))
                assert not st_off.route & PERIOD_BIT and ctx_off.period() == (0, 0, 0, 0)
                if n >= 1 << 16:
                    assert st.route & PERIOD_BIT and not st.route & RUN_BIT, (p, n, sp, st.route, line)
                    got_p, longest, votes, at = ctx.period()
                    assert got_p == p and longest > max(at, p) and at >= p and votes >= n // 64, (p, n, ctx.period())
                    assert line and line["stepped"] and line["p"] == p and line["at"] == at and line["passes"] == 1, line
                    bound = math.ceil(math.log2(max(1, p / line["depth"]))) + 3
                    assert st.rounds <= bound, (p, n, sp, st.rounds, bound, line)
                    if n >= 256 * max(p, line["depth"]):
                        assert st_off.rounds >= st.rounds + 6, (p, n, sp, st.rounds, st_off.rounds)


# ---- 2. types and ties --------------------------------------------------------------------

@pytest.mark.parametrize("extra", ["", "BWTC_HIP_GRAM_MIN_N=64"])
@pytest.mark.parametrize("p", [2, 3, 9, 64])
def test_types_and_ties(oracle, monkeypatch, p, extra):
    """Stretches of one unit that end in a smaller byte, a larger byte, the block's end and each other; equal (type, k)
    from 2, 3 and 64 stretches; units that are rotations of one another.  Plain keys and the long-key route."""
    blocks = pc.tie_blocks(p, 3000)
    stepped = 0
    with _contexts(monkeypatch, 1 << 20, extra, off=False) as (ctx, _):
        for i, (what, d) in enumerate(blocks):
            for sp in SPS:
                st = _same(ctx, d, sp, oracle.oracle_bwt_block(d, sp), (p, what, sp, extra))
            print("p %d %s: rounds %d route %#x period %s" % (p, what, st.rounds, st.route, ctx.period()))
            stepped += 1 if st.route & PERIOD_BIT else 0
    assert stepped * 2 > len(blocks), (stepped, len(blocks))          # the step under test ran


# ---- 3. around the gate -------------------------------------------------------------------

@pytest.mark.parametrize("p", [2, 3])
def test_stretches_around_the_gate(oracle, monkeypatch, capfd, p):
    """Noise with one planted stretch of max(d, p) - 1, max(d, p) and max(d, p) + 1 periodic characters, d the depth at
    which that block's rounds begin (from the debug line, checked again on every block).  The period is named
    (BWTC_HIP_PERIOD): a stretch that short collects no votes.  - 1 and 0 leave bit 8 clear and the rounds and
    active_sum as they are without the switch; + 1 takes the step."""
    with _contexts(monkeypatch, 1 << 20, "BWTC_HIP_PERIOD=%d" % p) as (ctx, ctx_off):
        d0 = pc.gate_block(p, 0)
        _, line, _ = _said(ctx, d0, 8, oracle.oracle_bwt_block(d0, 8), (p, "plain"), monkeypatch, capfd)
        depth = line["depth"]
        gate = max(depth, p)
        assert line["longest"] == pc.gate_block_longest(p, 0) < gate - 1, (line, gate)     # premise: the planted stretch is the longest
        print("p %d: the rounds begin at depth %d, the noise's longest stretch is %d" % (p, depth, line["longest"]))
        for delta in (-1, 0, 1):
            d = pc.gate_block(p, gate + delta)
            want = oracle.oracle_bwt_block(d, SPS[delta + 1])
            st, line, _ = _said(ctx, d, SPS[delta + 1], want, (p, delta), monkeypatch, capfd)
            assert line["depth"] == depth and line["longest"] == gate + delta and line["p"] == p, (p, delta, line)      # premise
            st_off = _same(ctx_off, d, SPS[delta + 1], want, (p, delta, "off"))
            assert not st_off.route & PERIOD_BIT
            if delta <= 0:
                assert not line["stepped"] and not st.route & PERIOD_BIT, (p, delta, line, st.route)
                assert st.rounds == st_off.rounds and st.active_sum == st_off.active_sum and st.route == st_off.route
            else:
                assert line["stepped"] and st.route & PERIOD_BIT and line["at"] == depth, (p, delta, line, st.route)
                assert ctx.period() == (p, gate + 1, 0, depth)


def test_period_below_at_and_above_the_depth(oracle, monkeypatch, capfd):
    """Units over five symbols -- the depth d at which the rounds begin does not depend on the period -- of d - 1, d and
    d + 1 bytes: a period up to d takes the first round as its step, a period above d a deferred step at the first
    depth that reaches it."""
    with _contexts(monkeypatch, 1 << 20, off=False) as (ctx, _):
        d5 = np.tile(pc.unit_of_five(5), 14000)
        _, line, _ = _said(ctx, d5, 8, oracle.oracle_bwt_block(d5, 8), "p 5", monkeypatch, capfd)
        depth = line["depth"]
        assert depth >= 6 and line["stepped"] and line["at"] == depth, line
        for p in (depth - 1, depth, depth + 1, 2 * depth, 2 * depth + 1):
            d = np.tile(pc.unit_of_five(p), 70000 // p)
            st, line, _ = _said(ctx, d, 8, oracle.oracle_bwt_block(d, 8), p, monkeypatch, capfd)
            print("depth %d, period %d: %s, rounds %d" % (depth, p, line, st.rounds))
            assert line["depth"] == depth and line["p"] == p and line["stepped"] and st.route & PERIOD_BIT, (p, line)     # premise: the same d
            if p <= depth:
                assert line["at"] == depth and st.rounds <= 3, (p, line, st.rounds)
            else:
                assert p <= line["at"] < 2 * p and line["at"] == depth * 2 ** math.ceil(math.log2(p / depth)), (p, line)
                assert st.rounds <= math.ceil(math.log2(p / depth)) + 3, (p, line, st.rounds)


# ---- 4. forced periods --------------------------------------------------------------------

def _run_and_period_block():
    d = np.tile(np.frombuffer(b"abcabcabd", np.uint8), 300000 // 9 + 1)[:300000].copy()
    d[100000:100000 + (1 << 16)] = 0
    return d


@pytest.mark.parametrize("forced", ["true", "double", "wrong", "one"])
def test_forced_periods(oracle, monkeypatch, forced):
    """BWTC_HIP_PERIOD = the true p, 2 p, a wrong p and 1 on blocks of cases 1 and 2: the bytes are right whatever the
    period.  Forced 1 is the run path: bit 8 stays clear, and bit 5 is set where the block holds a run above the depth
    (the block with a zero run; the stretches hold none)."""
    for p in (3, 64):
        value = {"true": p, "double": 2 * p, "wrong": p + 2, "one": 1}[forced]
        with _contexts(monkeypatch, 1 << 20, "BWTC_HIP_PERIOD=%d" % value, off=False) as (ctx, _):
            blocks = [("one stretch", pc.stretch(p, 1 << 16))] + pc.tie_blocks(p, 3000)
            blocks.append(("abab", pc.nonprimitive_block(6000)))
            blocks.append(("a run and a period", _run_and_period_block()))
            for what, d in blocks:
                for sp in (1, 8):
                    st = _same(ctx, d, sp, oracle.oracle_bwt_block(d, sp), (forced, p, what, sp))
                if forced == "one":
                    assert not st.route & PERIOD_BIT, (what, st.route)
                    if what == "a run and a period":
                        assert st.route & RUN_BIT, (what, st.route)
                elif what == "one stretch" and forced in ("true", "double"):
                    assert st.route & PERIOD_BIT and ctx.period()[0] == value, (what, st.route, ctx.period())
    if forced == "true":
        with _contexts(monkeypatch, 1 << 20, "BWTC_HIP_PERIOD=4", off=False) as (ctx, _):
            d = pc.nonprimitive_block(6000)
            st = _same(ctx, d, 8, oracle.oracle_bwt_block(d, 8), "abab with p = 4")
            assert st.route & PERIOD_BIT and ctx.period()[0] == 4, (st.route, ctx.period())


# ---- 5. routes ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _long_block(sigma):
    n = 300000 if sigma == 30 else 420000
    d = _words(n, sigma, sigma)
    d[20000:20000 + (1 << 18)] = np.tile(d[:7], (1 << 18) // 7 + 1)[:1 << 18]
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _long_want(sigma, sp):
    import oracle_lib
    return oracle_lib.oracle_bwt_block(_long_block(sigma), sp)


@pytest.mark.parametrize("extra", ["", "BWTC_HIP_TEXT_ROUNDS=0", "BWTC_HIP_LOCAL_ROUNDS=0", "BWTC_HIP_FINISHER=0", "BWTC_HIP_LONG=0",
                                   "BWTC_HIP_KEYS=grams", "BWTC_HIP_DENSE=0", "BWTC_HIP_RUNS=0"])
def test_long_key_route(oracle, monkeypatch, extra):
    """Blocks of random words over 30 and 200 symbols through the long-key route and its switches, with an embedded
    stretch of 2^18 bytes of period 7 (the block's first seven bytes): the period step runs and saves at least six
    rounds; premise: without it the block takes at least 10 (doubling from at most 2^8 characters to 2^18)."""
    with _contexts(monkeypatch, 1 << 20, "BWTC_HIP_GRAM_MIN_N=64," + extra) as (ctx, ctx_off):
        for i, sigma in enumerate((30, 200)):
            d, sp = _long_block(sigma), SPS[i]
            assert len(set(d[:7].tolist())) > 1
            st = _same(ctx, d, sp, _long_want(sigma, sp), (extra, sigma))
            st_off = _same(ctx_off, d, sp, _long_want(sigma, sp), (extra, sigma, "off"))
            print("%s sigma %d: rounds %d route %#x period %s against rounds %d route %#x"
                  % (extra, sigma, st.rounds, st.route, ctx.period(), st_off.rounds, st_off.route))
            assert st_off.rounds >= 10 and not st_off.route & PERIOD_BIT, (extra, sigma, st_off.rounds)
            assert st.route & PERIOD_BIT and not st.route & RUN_BIT, (extra, sigma, st.route, ctx.period())
            assert st.rounds + 6 <= st_off.rounds, (extra, sigma, st.rounds, st_off.rounds)


@functools.lru_cache(maxsize=None)
def _dense_block():
    d = np.random.default_rng(11).integers(0, 256, 4 << 20).astype(np.uint8)
    d[1 << 19:(1 << 19) + (3 << 20)] = np.tile(np.array([201, 17, 96], np.uint8), 1 << 20)
    d.setflags(write=False)
    import oracle_lib
    return d, oracle_lib.oracle_bwt_block(d, 8)


@pytest.mark.parametrize("extra", ["", "BWTC_HIP_LONG=0"])
def test_stretch_with_company_at_4MiB(oracle, monkeypatch, extra):
    """Random bytes with a 3 MiB stretch of period 3 in the middle: a list far above kPairsMin (the dense route).  At
    most five rounds; premise: at least 15 = log2(3 * 2^20 / 64) without the step."""
    d, want = _dense_block()
    with _contexts(monkeypatch, d.size, extra) as (ctx, ctx_off):
        st = _same(ctx, d, 8, want, extra)
        st_off = _same(ctx_off, d, 8, want, (extra, "off"))
        print("%s: rounds %d (route %#x, period %s) against %d (route %#x)" % (extra, st.rounds, st.route, ctx.period(), st_off.rounds, st_off.route))
        assert st_off.rounds >= 15, st_off.rounds
        assert st.route & PERIOD_BIT and st.rounds <= 5, (st.rounds, st.route)


def test_the_run_step_wins(oracle, monkeypatch):
    """A block with a long zero run and long stretches of period 9: one closed-form step per block, the run step."""
    d = _run_and_period_block()
    with _contexts(monkeypatch, 1 << 20, off=False) as (ctx, _):
        for sp in SPS:
            st = _same(ctx, d, sp, oracle.oracle_bwt_block(d, sp), sp)
            assert st.route & RUN_BIT and not st.route & PERIOD_BIT, st.route
            assert ctx.period() == (0, 0, 0, 0)


# ---- 6. nothing changes without periods ---------------------------------------------------

@pytest.mark.parametrize("name", ["random_bytes", "generator_text"])
def test_blocks_without_periods_take_the_same_rounds(oracle, monkeypatch, capfd, name):
    d = np.random.default_rng(3).integers(0, 256, 300000).astype(np.uint8) if name == "random_bytes" else synth.gen_text(1 << 20, 3)
    want = oracle.oracle_bwt_block(d, 8)
    with _contexts(monkeypatch, 1 << 20) as (ctx, ctx_off):
        st, line, _ = _said(ctx, d, 8, want, name, monkeypatch, capfd)
        st_off = _same(ctx_off, d, 8, want, (name, "off"))
        assert not st.route & PERIOD_BIT and st.route == st_off.route, (st.route, st_off.route)
        assert st.rounds == st_off.rounds and st.active_sum == st_off.active_sum, (st.rounds, st_off.rounds, st.active_sum, st_off.active_sum)
        assert ctx.period()[0] == 0 and ctx.period()[1] == 0 and ctx.period()[3] == 0, ctx.period()
        assert line is None or (not line["stepped"] and line["passes"] == 0), line          # no period-length pass was launched


# ---- 7. randomised ------------------------------------------------------------------------

def test_random_period_blocks(oracle, monkeypatch):
    """100 blocks of stretches of mixed periods, 1 included, and noise; every fourth block twice its first half.  Every
    other block goes through the long-key route; the two contexts are reused throughout."""
    stepped = ran = 0
    with _contexts(monkeypatch, 1 << 20, off=False) as (ctx_plain, _), \
            _contexts(monkeypatch, 1 << 20, "BWTC_HIP_GRAM_MIN_N=64", off=False) as (ctx_long, _):
        for it in range(100):
            ctx = ctx_long if it % 2 else ctx_plain
            d, sp = pc.random_block(it)
            st = _same(ctx, d, sp, oracle.oracle_bwt_block(d, sp), (it, d.size, sp))
            stepped += 1 if st.route & PERIOD_BIT else 0
            ran += 1 if st.route & RUN_BIT else 0
    print("%d period steps, %d run steps" % (stepped, ran))
    assert stepped >= 12 and ran >= 12, (stepped, ran)
