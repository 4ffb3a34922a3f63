"""The suffix sorter's run step on the GPU (-m gpu): blocks with long runs of one byte, every result -- bytes, LF
powers, freqs -- against oracle.oracle_bwt_block, and the number of rounds (bwtc_hip_stats.rounds, route bit 5) where
the step is the point.  A switch is read when a context is made, so every test opens its own contexts: one as
shipped and, where rounds are compared, one with BWTC_HIP_RUNS=0 (the sorter without the step).

Without the run step the asserts on `route & 32` and on the rounds of cases 1, 4 and 5 fail: a run of L bytes then
takes log2(L / depth) doubling rounds."""
import contextlib
import functools
import math
import re

import numpy as np
import pytest

from bwtc_amd import synth

pytestmark = pytest.mark.gpu

RUN_BIT = 32
SPS = (1, 2, 8, 256)
DEBUG_LINE = re.compile(r"runs: longest run (\d+), the rounds begin at depth (\d+): (run step|no run step)")


@contextlib.contextmanager
def _contexts(monkeypatch, size, extra="", off=True):
    """(context as shipped, context with BWTC_HIP_RUNS=0 or None), both with the switches of `extra`."""
    from bwtc_amd import hip
    for one in extra.split(","):
        if one:
            name, value = one.split("=")
            monkeypatch.setenv(name, value)
    monkeypatch.delenv("BWTC_HIP_RUNS", raising=False)
    ctx_on = hip.Context(0, size)
    ctx_off = None
    if off:
        monkeypatch.setenv("BWTC_HIP_RUNS", "0")
        ctx_off = hip.Context(0, size)
        monkeypatch.delenv("BWTC_HIP_RUNS")
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


def _words(n, sigma, seed, lowest=1):
    """Random words over sigma symbols (none below `lowest`), n bytes."""
    rng = np.random.default_rng(seed)
    alphabet = rng.choice(np.arange(lowest, 256), sigma, replace=False).astype(np.uint8)
    words = [alphabet[rng.integers(0, sigma, int(rng.integers(1, 9)))] for _ in range(150)]
    return np.concatenate([words[int(i)] for i in rng.integers(0, len(words), n // 3 + 8)])[:n].copy()


# ---- 1. one run ---------------------------------------------------------------------------

@pytest.mark.parametrize("byte", [0, 0xFF])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4096, 1 << 20, (1 << 22) + 3])
def test_one_run(oracle, monkeypatch, n, byte):
    """A block that is one run.  From 4096 bytes up the run step must have run and at most two rounds are left, where
    doubling alone needs at least log2(n / 64) (the deepest initial key holds 64 characters).  (2^22 + 3 bytes: a list
    above kPairsMin = 2^21 entries, and a block the long-key route takes.)"""
    d = np.full(n, byte, np.uint8)
    sps = SPS
    with _contexts(monkeypatch, n, off=False) as (ctx, _):
        for sp in sps:
            st = _same(ctx, d, sp, oracle.oracle_bwt_block(d, sp), (n, byte, sp))
            print("one run of %d x %#x, %d starting points: rounds %d route %#x" % (n, byte, sp, st.rounds, st.route))
            if n >= 4096:
                assert math.log2(n / 64) >= 6
                assert st.route & RUN_BIT and st.rounds <= 2, (n, byte, sp, st.rounds, st.route)


# ---- 2. types and ties --------------------------------------------------------------------

def _tie_blocks():
    rng = np.random.default_rng(77)
    L = 3000
    out = []

    def filler(n, lowest=1):
        return rng.integers(lowest, 256, n).astype(np.uint8)

    def cat(*parts):
        return np.concatenate([np.asarray(p, np.uint8).ravel() for p in parts])

    for c in (0x50, 0):
        run = np.full(L, c, np.uint8)
        sides = {"absent": [], "below": [c - 1] if c else None, "above": [c + 1]}
        for xn, x in sides.items():
            for yn, y in sides.items():
                if x is None or y is None:
                    continue                      # nothing lies below zero
                out.append(("c=%d x %s y %s, at the block's ends" % (c, xn, yn), cat(x, run, y)))
                out.append(("c=%d x %s y %s, inside" % (c, xn, yn), cat(filler(2000, 1), x, run, y, filler(2000, 1))))
                out.append(("c=%d x %s y %s, inside, other zero bytes" % (c, xn, yn), cat(filler(2000, 0), [0], x, run, y, filler(2000, 0))))
    c = 0x50
    run = np.full(L, c, np.uint8)
    out.append(("two equal runs, tails below and above", cat(filler(500), run, [c - 9], filler(500), run, [c + 9], filler(500))))
    out.append(("three equal runs, different tails", cat(run, [3], run, [200], run, [4], filler(300), [c + 1], run, [c - 1], run)))
    for shared in (1, 100, 5000):
        tail = _words(shared, 30, shared)
        # (the block is reversed for sorting: what follows a run in T precedes it in the block)
        out.append(("equal runs, tails share %d characters" % shared,
                    cat([7], tail, run, filler(50), [9], tail, run, filler(50), [8], tail, run, [11], tail[::-1], run, [12], tail[::-1], run)))
    out.append(("runs that differ in length by one", cat(filler(100), run, [1], run[:-1], [1], run, [c], [250], run[:-2], [250], run[:-1])))
    low = 9
    body = filler(3000, low)
    lowrun = np.full(L, low, np.uint8)
    out.append(("the smallest byte's run begins the block: the terminator follows it in T", cat(lowrun, [low + 5], body, lowrun, body)))
    out.append(("the smallest byte's run ends the block", cat(body, lowrun, [low + 5], body, lowrun)))
    zrun = np.zeros(L, np.uint8)
    out.append(("a zero run begins the block: the terminator joins it", cat(zrun, body, zrun, [1], body)))
    out.append(("a zero run begins and ends the block, no other zero", cat(zrun, body, zrun)))
    out.append(("zero runs and single zero bytes", cat(zrun, filler(3000, 0), zrun[:-1], filler(3000, 0), zrun)))
    return out


@pytest.mark.parametrize("extra", ["", "BWTC_HIP_GRAM_MIN_N=64"])
def test_types_and_ties(oracle, monkeypatch, extra):
    """x c^L y for x and y below, above and absent, at the block's ends and inside; equal runs whose tails differ at
    once or after 1, 100 and 5000 shared characters (their ranks are unsettled at the run step); lengths that differ by
    one; the terminator joining a run or following the smallest byte's run, whose key code it shares; c = 0 with and
    without other zero bytes (both plans of the terminator's code).  Plain keys and the long-key route."""
    blocks = _tie_blocks()
    stepped = 0
    with _contexts(monkeypatch, 1 << 20, extra, off=False) as (ctx, _):
        for i, (what, d) in enumerate(blocks):
            for sp in SPS:
                st = _same(ctx, d, sp, oracle.oracle_bwt_block(d, sp), (what, sp, extra))
            stepped += 1 if st.route & RUN_BIT else 0
    assert stepped * 2 > len(blocks), (stepped, len(blocks))          # the step under test ran


# ---- 3. around the depth ------------------------------------------------------------------

def _depth_block(kind, run):
    rng = np.random.default_rng(5)
    if kind == "bytes":                            # 256 symbols: keys of 4 characters
        d = rng.integers(1, 256, 1000000).astype(np.uint8)          # (enough suffixes for some to tie on four characters)
        d[d == 77] = 78
        c = 77
    elif kind == "four":                           # 4 symbols: keys of 16 characters
        d = np.array([65, 67, 71, 84], np.uint8)[rng.integers(0, 4, 1000000)]
        d[np.flatnonzero((d[1:] == 84) & (d[:-1] == 84)) + 1] = 65        # no run of the planted symbol but the planted one
        c = 84
    else:                                          # long keys: words, and a period of thousands (a group the finisher leaves to the rounds)
        d = _words(300000, 30, 3)
        d[d == 77] = 78
        d[100000:130000] = np.tile(np.array([31, 32, 33, 34, 35, 36, 37], np.uint8), 5000)[:30000]
        c = 77
    if run:
        d[50000:50000 + run] = c
        d[49999] = d[50000 + run] = 65 if kind == "four" else c + 1       # (a symbol the block holds anyway: the same key plan)
    return d


@pytest.mark.parametrize("kind,extra", [("bytes", ""), ("four", ""), ("long", "BWTC_HIP_GRAM_MIN_N=64")])
def test_runs_around_the_depth(oracle, monkeypatch, capfd, kind, extra):
    """Runs of d - 1, d and d + 1 bytes, d = the depth at which that block's rounds begin, read from the sorter's own
    debug line (and checked again on every block: the premise).  d - 1 must leave the route bit clear and the rounds
    as they are without the switch; d + 1 must take the step."""
    def run(ctx, d, sp, debug):
        if debug:
            monkeypatch.setenv("BWTC_HIP_DEBUG", "1")
            capfd.readouterr()
        st = _same(ctx, d, sp, oracle.oracle_bwt_block(d, sp), (kind, sp))
        if not debug:
            return st, None
        monkeypatch.delenv("BWTC_HIP_DEBUG")
        lines = DEBUG_LINE.findall(capfd.readouterr().err)
        assert len(lines) == 1, lines
        return st, (int(lines[0][0]), int(lines[0][1]), lines[0][2])

    with _contexts(monkeypatch, 1 << 20, extra) as (ctx, ctx_off):
        _, (longest0, depth, _) = run(ctx, _depth_block(kind, 0), 8, True)
        assert longest0 < depth - 1, (longest0, depth)               # premise: the planted run is the block's longest
        print("%s: the rounds begin at depth %d (longest run of the plain block: %d)" % (kind, depth, longest0))
        for delta in (-1, 0, 1):
            d = _depth_block(kind, depth + delta)
            st, (longest, depth_now, said) = run(ctx, d, SPS[delta + 1], True)
            assert depth_now == depth and longest == depth + delta, (kind, delta, depth, depth_now, longest)      # premise
            st_off, _ = run(ctx_off, d, SPS[delta + 1], False)
            assert not st_off.route & RUN_BIT
            if delta < 0:
                assert said == "no run step" and not st.route & RUN_BIT, (kind, delta, said, st.route)
                assert st.rounds == st_off.rounds and st.active_sum == st_off.active_sum
            if delta > 0:
                assert said == "run step" and st.route & RUN_BIT, (kind, delta, said, st.route)


# ---- 4. long-key route --------------------------------------------------------------------

LONG_BLOCKS = ("run_2pow18", "runs_200x300", "run_200", "giant")


@functools.lru_cache(maxsize=None)
def _long_block(sigma, name):
    n = 300000 if sigma == 30 else 420000
    d = _words(n, sigma, sigma)
    rng = np.random.default_rng(sigma + 1)
    c = int(d[0])
    if name == "run_2pow18":                       # a hard group: 2^18 members
        d[20000:20000 + (1 << 18)] = c
    elif name == "runs_200x300":                   # groups of at most 300 members: the finisher's
        for a in rng.choice(np.arange(0, n - 400, 400), 200, replace=False):
            d[a:a + 300] = rng.choice(d[:50])
    elif name == "run_200":
        d[1000:1200] = c
    else:                                          # groups of tens of thousands of members: the finisher is skipped
        d[:] = np.tile(np.frombuffer(b"abcabcabd", np.uint8), n // 9 + 1)[:n]
        d[100000:100000 + (1 << 16)] = 0
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _long_want(sigma, name, sp):
    import oracle_lib
    return oracle_lib.oracle_bwt_block(_long_block(sigma, name), sp)


@pytest.mark.parametrize("extra", ["", "BWTC_HIP_TEXT_ROUNDS=0", "BWTC_HIP_LOCAL_ROUNDS=0", "BWTC_HIP_FINISHER=0", "BWTC_HIP_LONG=0",
                                   "BWTC_HIP_KEYS=grams", "BWTC_HIP_DENSE=0", "BWTC_HIP_SORT=sweep"])
def test_long_key_route(oracle, monkeypatch, capfd, extra):
    """Blocks of random words over 30 and 200 symbols through the long-key route and its switches: an embedded run of
    2^18 bytes (a hard group), 200 runs of 300 bytes and one of 200 (groups the finisher keeps), and a block whose groups
    are so large that the finisher is skipped.  The 2^18 run: the run step runs and saves at least six rounds; premise:
    without it the block takes at least 10 (doubling from a depth of at most 2^8 characters to 2^18).  The last block's
    premise -- more than 64 members per group, the finisher skipped -- is read from the sorter's debug line wherever
    the finisher route is taken."""
    with _contexts(monkeypatch, 1 << 20, "BWTC_HIP_GRAM_MIN_N=64," + extra) as (ctx, ctx_off):
        for i, (sigma, name) in enumerate((s, b) for s in (30, 200) for b in LONG_BLOCKS):
            d, sp = _long_block(sigma, name), SPS[i % 4]
            if name == "giant":
                monkeypatch.setenv("BWTC_HIP_DEBUG", "1")
                capfd.readouterr()
            st = _same(ctx, d, sp, _long_want(sigma, name, sp), (extra, sigma, name))
            if name == "giant":
                monkeypatch.delenv("BWTC_HIP_DEBUG")
                said = capfd.readouterr().err
                if st.route & 1 and "FINISHER" not in extra:
                    assert "finisher: skipped" in said, (extra, sigma, said[-2000:])
            print("%s sigma %d %s: rounds %d active_sum %d route %#x" % (extra, sigma, name, st.rounds, st.active_sum, st.route))
            if name == "run_2pow18":
                st_off = _same(ctx_off, d, sp, _long_want(sigma, name, sp), (extra, sigma, name, "off"))
                print("   without the step: rounds %d active_sum %d route %#x" % (st_off.rounds, st_off.active_sum, st_off.route))
                assert st_off.rounds >= 10 and not st_off.route & RUN_BIT, (extra, sigma, st_off.rounds)
                assert st.route & RUN_BIT and st.rounds + 6 <= st_off.rounds, (extra, sigma, st.rounds, st_off.rounds, st.route)


# ---- 5. dense route with company ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _dense_block():
    d = np.random.default_rng(11).integers(0, 256, 4 << 20).astype(np.uint8)
    d[1 << 19:(1 << 19) + (3 << 20)] = 0
    d.setflags(write=False)
    import oracle_lib
    return d, oracle_lib.oracle_bwt_block(d, 8)


@pytest.mark.parametrize("extra", ["", "BWTC_HIP_LONG=0"])
def test_run_with_company_at_4MiB(oracle, monkeypatch, extra):
    """Random bytes with a 3 MiB zero run in the middle: a list far above kPairsMin (the dense route without the long
    keys).  At most four rounds; premise: at least 15 = log2(3 * 2^20 / 64) without the step."""
    d, want = _dense_block()
    with _contexts(monkeypatch, d.size, extra) as (ctx, ctx_off):
        st = _same(ctx, d, 8, want, extra)
        st_off = _same(ctx_off, d, 8, want, (extra, "off"))
        print("%s: rounds %d (route %#x) against %d (route %#x)" % (extra, st.rounds, st.route, st_off.rounds, st_off.route))
        assert st_off.rounds >= 15, st_off.rounds
        assert st.route & RUN_BIT and st.rounds <= 4, (st.rounds, st.route)


# ---- 6. nothing changes without runs ------------------------------------------------------

@pytest.mark.parametrize("name", ["period_9", "random_bytes", "generator_text"])
def test_blocks_without_runs_take_the_same_rounds(oracle, monkeypatch, name):
    if name == "period_9":
        d = np.tile(np.frombuffer(b"abcabcabd", np.uint8), 30000)
    elif name == "random_bytes":
        d = np.random.default_rng(3).integers(0, 256, 300000).astype(np.uint8)
    else:
        d = synth.gen_text(1 << 20, 3)
    want = oracle.oracle_bwt_block(d, 8)
    with _contexts(monkeypatch, 1 << 20) as (ctx, ctx_off):
        st = _same(ctx, d, 8, want, name)
        st_off = _same(ctx_off, d, 8, want, (name, "off"))
        assert not st.route & RUN_BIT and st.route == st_off.route, (st.route, st_off.route)
        assert st.rounds == st_off.rounds and st.active_sum == st_off.active_sum, (st.rounds, st_off.rounds, st.active_sum, st_off.active_sum)


# ---- 7. randomised ------------------------------------------------------------------------

def _random_block(it, depth):
    """Block `it` of the randomised case; depth (or None): the depth its rounds begin at, for the runs of depth +- 1."""
    rng = np.random.default_rng([20240611, it])
    lengths = [1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 70000]
    if depth:
        lengths += [max(1, depth - 1), depth + 1] * 3
    alphabets = [np.array([0], np.uint8), np.array([0, 255], np.uint8), np.array([0, 1, 200], np.uint8),
                 np.arange(40, 70, dtype=np.uint8)]
    n = int(300 * (400000 / 300) ** rng.random())
    alphabet = alphabets[int(rng.integers(0, 4))]
    twice = it % 3 == 0
    sp = SPS[int(rng.integers(0, 4))]
    target = n // 2 if twice else n
    parts, have = [], 0
    while have < target:
        lens = rng.choice(lengths, 4096)
        if alphabet.size > 2:                      # mostly short runs, so that the long ones have company
            lens = np.where(rng.random(4096) < 0.7, rng.choice([1, 2, 3], 4096), lens)
        parts.append(np.repeat(alphabet[rng.integers(0, alphabet.size, 4096)], lens))
        have += parts[-1].size
    d = np.concatenate(parts)[:target]
    return (np.concatenate([d, d]) if twice else d), sp


@pytest.mark.parametrize("part", range(4))
def test_random_run_blocks(oracle, monkeypatch, capfd, part):
    """120 blocks (four parts of 30, one seed) of 300 ... 400 000 bytes (sizes drawn evenly in the logarithm) built from
    runs over {0}, {0, 255}, 3 and 30 symbols; run lengths from 1, 2, 3, d +- 1, 255-257, 4095-4097 and 70 000; a third
    of the blocks repeated twice.  Every other block goes through the long-key route.  d is the block's own: the depth
    its rounds begin at, read from the sorter's debug line; the block is drawn again with runs of d +- 1 until the line
    names the d it was drawn with (the premise, asserted)."""
    def depth_of(ctx, d, sp):
        monkeypatch.setenv("BWTC_HIP_DEBUG", "1")
        capfd.readouterr()
        ctx.bwt_block(d, sp)
        monkeypatch.delenv("BWTC_HIP_DEBUG")
        lines = DEBUG_LINE.findall(capfd.readouterr().err)
        return int(lines[0][1]) if lines else None

    stepped = with_depth = 0
    with _contexts(monkeypatch, 1 << 20, off=False) as (ctx_plain, _), \
            _contexts(monkeypatch, 1 << 20, "BWTC_HIP_GRAM_MIN_N=64", off=False) as (ctx_long, _):
        for it in range(30 * part, 30 * part + 30):
            ctx = ctx_long if it % 2 else ctx_plain
            depth = None
            for attempt in range(5):
                d, sp = _random_block(it, depth)
                now = depth_of(ctx, d, sp)
                if now == depth:
                    break
                depth = now
            assert now == depth, (it, depth, now)                     # premise: the runs of d +- 1 are around this block's d
            with_depth += 1 if depth else 0
            st = _same(ctx, d, sp, oracle.oracle_bwt_block(d, sp), (it, d.size, depth, sp))
            stepped += 1 if st.route & RUN_BIT else 0
    assert stepped >= 10 and with_depth >= 10, (stepped, with_depth)


# ---- 7b. a run step beside a live local list ------------------------------------------------

def test_run_step_beside_the_local_list(oracle, monkeypatch):
    """Deep repeats in small groups (3 MiB of the generator's text three times: the local list, route bit 6) and a run
    of 70 000 zeros inside the repeated piece: three equal runs whose tails are the same text for megabytes, members of
    local groups whose ranks are only as deep as the local list.  The run step must not let the rounds look deeper
    than those ranks reach."""
    size = 16 << 20
    d = synth.gen_text(size, 77)
    d[1 << 20:(1 << 20) + 70000] = 0
    d[5 << 20:8 << 20] = d[:3 << 20]
    d[11 << 20:14 << 20] = d[:3 << 20]
    want = oracle.ref_bwt_block(d, 8) if oracle.ref() is not None else oracle.oracle_bwt_block(d, 8)
    with _contexts(monkeypatch, size) as (ctx, ctx_off):
        st = _same(ctx, d, 8, want, "on")
        st_off = _same(ctx_off, d, 8, want, "off")
        print("rounds %d route %#x against %d route %#x" % (st.rounds, st.route, st_off.rounds, st_off.route))
        assert st.route & 64 and st.route & RUN_BIT, st.route           # premise: the local list was live, the step ran
        assert st.rounds <= st_off.rounds + 1, (st.rounds, st_off.rounds)


# ---- 8. one context reused ----------------------------------------------------------------

def test_one_context_reused(oracle, monkeypatch):
    """Run block, block without runs, smaller run block, a refused size, run block: nothing of a block's runs -- k[],
    the depth of its run step, the gate -- may reach the next."""
    from bwtc_amd import hip
    rng = np.random.default_rng(8)
    big = rng.integers(1, 256, 200000).astype(np.uint8)
    big[30000:130000] = 5
    plain = rng.integers(0, 256, 200000).astype(np.uint8)
    small = rng.integers(1, 256, 20000).astype(np.uint8)
    small[100:9000] = 200
    small[12000:19000] = 200
    again = rng.integers(0, 256, 150000).astype(np.uint8)
    again[:60000] = 0
    again[70000:120000] = 255
    with _contexts(monkeypatch, 200000, off=False) as (ctx, _):
        for what, d, stepped in (("run", big, True), ("plain", plain, False), ("smaller run", small, True), ("refused", None, None),
                                 ("run again", again, True), ("plain again", plain, False)):
            if d is None:
                with pytest.raises(hip.BwtcHipError):
                    ctx.bwt_block(np.zeros((1 << 20) + 4096, np.uint8), 8)           # (the smallest context holds 2^20 bytes)
                continue
            for sp in (8, 1):
                st = _same(ctx, d, sp, oracle.oracle_bwt_block(d, sp), (what, sp))
                assert bool(st.route & RUN_BIT) == stepped, (what, sp, st.route)
