"""The device postprocessor (postprocess.hip behind bwtc_hip_postprocess_device / _block) at its grammar, tile,
seam and size limits.

Grammars are hand-built by tests/pgrammar.py (variables of exact lengths, sixteen special symbols, pairs that
stand for nothing); the expected bytes come from its model, which test_pgrammar.py holds against the oracle and
the host function on everything up to MEDIUM bytes of output, and from closed forms (np.tile of one token) above.
All comparisons are exact.  Every device call runs on a buffer with a guard in front of and behind the output and
behind the input, at chosen offsets from 16-byte alignment, asserts its route, and its statistics are checked
against what the model says: tokens, pair tokens, pool bytes, output bytes and launches
((3 with special symbols else 1) + (1 scan launch up to 4096 tiles else 2) + 1 write).

A capacity above the output's size is a bound only: the tests rely on the entry points never touching more than
the bytes they produce, and the guards check it.  The project refuses a grammar one of whose rules stands for more
than `cap` bytes (or all together for more than 2 cap + 2^20), so cases whose output is smaller than their longest
rule pass cap = Model.min_cap()."""
import ctypes
import time

import numpy as np
import pytest

import pgrammar
from bwtc_amd import hip
from test_pgrammar import MEDIUM

pytestmark = pytest.mark.gpu
GUARD = 4096
FILL = 0xC3
TILE = 4096
IN_OFFSETS = (0, 1, 8, 15)


@pytest.fixture(scope="module")
def ctx():
    with hip.Context(0, 16 << 20) as c:
        yield c


def _loaded(kit):
    g = hip.Grammar()
    raw = kit.grammar()
    assert g.read(raw) == raw.size
    return g, kit.model()


def _launches(model, n, size):
    if n == 0 or model.n_rules == 0:
        return 0
    tiles = -(-n // TILE)
    return (3 if model.specials else 1) + (1 if tiles <= 4096 else 2) + (1 if size else 0)


def _check_stats(st, model, data, size, route=1):
    assert st["route"] == route and st["in_bytes"] == data.size and st["out_bytes"] == size, st
    if route != 1:
        return
    tokens, pairs = pgrammar.token_counts(model, data)
    if model.n_rules == 0:
        assert st["tokens"] == data.size and st["pair_tokens"] == 0 and st["launches"] == 0, st
        return
    assert st["tokens"] == tokens and st["pair_tokens"] == pairs, (st, tokens, pairs)
    assert st["pool_bytes"] == model.pool_bytes, (st, model.pool_bytes)
    assert st["launches"] == _launches(model, data.size, size), (st, _launches(model, data.size, size))
    assert st["workspace_bytes"] >= (2 * pgrammar.KEYS + 8) * 4 + model.pool_bytes + 8 * (-(-data.size // TILE)), st


def _same(got, want, what):
    assert got.size == want.size, (what, got.size, want.size)
    if not (got == want).all():
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s: first difference at output byte %d (got %d, want %d), %d bytes differ"
                             % (what, at, got[at], want[at], int((got != want).sum())))


class Arena:
    """Device buffers for one input: the input at d_in + in_off with a guard behind it, the output at
    d_out + GUARD + out_off with a guard before and behind it."""

    def __init__(self, ctx, n, size):
        self.ctx, self.n, self.size = ctx, n, size
        self.d_in = ctx.dmalloc(16 + n + GUARD)
        self.d_out = ctx.dmalloc(GUARD + 16 + size + GUARD)

    def close(self):
        self.ctx.dfree(self.d_in)
        self.ctx.dfree(self.d_out)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def run(self, g, data, cap, in_off=0, out_off=0):
        """(return code or bytes produced, the output buffer as it was left from the start of the front guard)"""
        ctx = self.ctx
        src = np.full(16 + self.n + GUARD, FILL, np.uint8)
        src[in_off:in_off + self.n] = data
        ctx.to_device(self.d_in, src)
        ctx.to_device(self.d_out, np.full(GUARD + 16 + self.size + GUARD, FILL, np.uint8))
        try:
            n_out = ctx.postprocess_device(g, self.d_in + in_off, self.n, self.d_out + GUARD + out_off, cap)
        except hip.BwtcHipError as e:
            n_out = e.code
        assert (ctx.to_host(self.d_in, src.size) == src).all(), "the input or the guard behind it was written"
        return n_out, ctx.to_host(self.d_out, GUARD + 16 + self.size + GUARD)


def _expect(model, data, og=None, oracle=None):
    want = pgrammar.expand(model, data)
    if og is not None and want.size <= MEDIUM:
        ref = oracle.oracle_postprocess(og, data, max(want.size, model.min_cap()) + 8)
        assert ref is not None and ref.tobytes() == want.tobytes()
    return want


def _device_case(ctx, g, model, data, want, placements, what, cap=None, route=1):
    """postprocess_device of `data` at every (in_off, out_off) of `placements`: bytes, guards, route, statistics."""
    cap = max(want.size, model.min_cap()) if cap is None else cap
    st = None
    with Arena(ctx, data.size, want.size) as arena:
        for in_off, out_off in placements:
            n_out, back = arena.run(g, data, cap, in_off, out_off)
            a = GUARD + out_off
            assert n_out == want.size, (what, in_off, out_off, n_out, want.size)
            assert (back[:a] == FILL).all(), (what, in_off, out_off, "the guard before the output was written")
            assert (back[a + n_out:] == FILL).all(), (what, in_off, out_off, "bytes behind the output were written")
            _same(back[a:a + n_out], want, "%s in+%d out+%d" % (what, in_off, out_off))
            st = ctx.postprocess_stats()
            _check_stats(st, model, data, want.size, route)
    return st


def _block_case(ctx, g, model, data, want, what, cap=None, route=1):
    """bwtc_hip_postprocess_block into a host buffer of the real size with a guard behind it."""
    cap = max(want.size, model.min_cap()) if cap is None else cap
    data = np.ascontiguousarray(data, np.uint8)
    out = np.full(want.size + GUARD, FILL, np.uint8)
    n = hip._u64(0)
    rc = ctx.lib.bwtc_hip_postprocess_block(ctx.handle, g.h, hip._ptr(data) if data.size else hip._ptr(out), data.size, hip._ptr(out), cap,
                                            ctypes.byref(n))
    assert rc == 0 and n.value == want.size, (what, rc, n.value, want.size)
    assert (out[want.size:] == FILL).all(), (what, "bytes behind the output were written")
    _same(out[:want.size], want, what + " (block)")
    st = ctx.postprocess_stats()
    _check_stats(st, model, data, want.size, route)
    return st


def _placements(size):
    if size <= 1 << 16:
        return [(i, o) for i in range(16) for o in range(16)]
    return [(IN_OFFSETS[o % 4], o) for o in range(16)]


# ---- a. token lengths and the output's phase -------------------------------------------------------------

@pytest.mark.parametrize("L", pgrammar.TOKEN_LENGTHS)
def test_token_lengths_at_every_phase(ctx, oracle, L):
    """Gap 3 (long expansions in k_pp_write) and gap 4 (pointers off 16-byte alignment), statistics exact (gap 8)."""
    kit, var, others = pgrammar.length_grammar(L)
    g, model = _loaded(kit)
    og = oracle.OracleGrammar()
    og.read(kit.grammar())
    assert len(model.of(var)) == L
    rng = np.random.default_rng(L)
    x, y, z = pgrammar.PLAIN
    short = list(others.values()) + [x, y, z]
    cases = [("alone", pgrammar.symbols([var])),
             ("between", pgrammar.symbols([x, var, y])),
             ("mix", pgrammar.long_mix(rng, short, var, L))]
    small = [v for m, v in others.items() if m <= 33] + [x, y, z] * 3 + ([var] if L <= 4097 else [])
    for n in (4095, 4096, 4097, 8193):
        cases.append(("tiles_%d" % n, pgrammar.mix(rng, small, n)))
    for name, data in cases:
        want = _expect(model, data, og, oracle)
        st = _device_case(ctx, g, model, data, want, _placements(want.size), "L=%d %s" % (L, name))
        if name in ("alone", "between", "mix"):
            _block_case(ctx, g, model, data, want, "L=%d %s" % (L, name))
        if L == (1 << 20) + 1:
            print("L=2^20+1 %s: %d bytes out, ms_device %.3f" % (name, want.size, st["ms_device"]))
    data = cases[2][1]
    lens = model.key_len[pgrammar.token_keys(model, data)[0]]
    assert lens.size >= 300 and (L == 1 or (lens == L).sum() >= 3)
    assert np.unique((np.cumsum(lens) - lens) % 16).size == 16, "token boundaries at every offset within a group"


# ---- b. special runs and seams ------------------------------------------------------------------------------

def _special(ctx, oracle):
    kit = pgrammar.special_kit()
    g, model = _loaded(kit)
    og = oracle.OracleGrammar()
    og.read(kit.grammar())
    return kit, g, model, og


def _run(rng, k):
    sp = np.array(pgrammar.SPECIALS, np.uint8)
    return sp[rng.integers(0, sp.size, k)]


def _random_bytes(rng, model, n):
    """Uniformly random bytes, except that a byte that stands for more than 64 bytes becomes a plain one (the output
    stays within a few times the input; pairs of any length stay in)."""
    data = rng.integers(0, 256, n, dtype=np.uint8)
    data[model.key_len[data] > 64] = pgrammar.PLAIN[0]
    return data


def _plain_filler(rng, kit, k):
    """k bytes none of which is special: plain bytes and byte variables"""
    pool = np.array(list(pgrammar.PLAIN) + [v for v in kit.length if not isinstance(v, tuple)] + list(pgrammar.FREED), np.uint8)
    return pool[rng.integers(0, pool.size, k)]


def test_pairs_across_tile_seams(ctx, oracle):
    """Gap 4/6 neighbours: a pair whose first byte is a tile's last, at both parities of the run, at several seams."""
    kit, g, model, og = _special(ctx, oracle)
    rng = np.random.default_rng(41)
    for seam in (TILE, 2 * TILE, 5 * TILE):
        for before in (1, 2, 3):                               # the run starts this many bytes before the seam
            for length in (2, 3, 4, 7, TILE, TILE + 1, 2 * TILE + 3):
                data = np.concatenate([_plain_filler(rng, kit, seam - before), _run(rng, length), _plain_filler(rng, kit, 9)])
                want = _expect(model, data, og, oracle)
                _device_case(ctx, g, model, data, want, [(0, 0), (1, 15), (15, 7)], "seam %d-%d run %d" % (seam, before, length))
    data = np.concatenate([_plain_filler(rng, kit, TILE - 1), _run(rng, 2), _plain_filler(rng, kit, TILE - 2), _run(rng, 3)])
    want = _expect(model, data, og, oracle)
    _device_case(ctx, g, model, data, want, _placements(1 << 20), "two seams")
    _block_case(ctx, g, model, data, want, "two seams")


def test_blocks_of_special_bytes_only(ctx, oracle):
    """Every tile's mark is 0: the run starts at 0 for all of them."""
    kit, g, model, og = _special(ctx, oracle)
    rng = np.random.default_rng(42)
    for n in (1, 2, 5000, 5001, 3 * TILE, 3 * TILE + 1, 40 * TILE + 1):
        data = _run(rng, n)
        want = _expect(model, data, og, oracle)
        _device_case(ctx, g, model, data, want, [(0, 0), (8, 1), (1, 8)], "special only %d" % n)
        _block_case(ctx, g, model, data, want, "special only %d" % n)
        assert pgrammar.token_counts(model, data) == ((n + 1) // 2, n // 2)


def test_last_byte_special_and_alone(ctx, oracle):
    kit, g, model, og = _special(ctx, oracle)
    rng = np.random.default_rng(43)
    for n in (TILE, TILE + 1, 3 * TILE, 3 * TILE + 1):
        for run in (1, 3, TILE - 1, TILE + 1):                  # odd: the last byte of the run starts a token
            if run >= n:
                continue
            data = np.concatenate([_plain_filler(rng, kit, n - run), _run(rng, run)])
            assert data.size == n
            want = _expect(model, data, og, oracle)
            keys, _ = pgrammar.token_keys(model, data)
            assert keys[-1] == data[-1], "the last token is the special byte alone"
            _device_case(ctx, g, model, data, want, [(0, 0), (15, 15), (1, 3)], "last special n=%d run=%d" % (n, run))
            _block_case(ctx, g, model, data, want, "last special n=%d run=%d" % (n, run))


@pytest.mark.parametrize("end_tile", [1500, 2100])
def test_special_runs_across_head_scan_chunks(ctx, oracle, end_tile):
    """Gap 1: k_pr_head_scan's carry over chunks of 1024 tiles.  The run starts at an odd position in tile 5 and ends
    in tile 1500 (one chunk seam) or 2100 (two, input above 8 MiB): for the first tile of each later chunk
    (tile start - true run start) is odd, so a carry that is lost (run start 0) changes the tokens."""
    kit, g, model, og = _special(ctx, oracle)
    rng = np.random.default_rng(end_tile)
    start = 5 * TILE + 1
    run = _run(rng, end_tile * TILE + 7 - start)
    data = np.concatenate([_plain_filler(rng, kit, start), run, _plain_filler(rng, kit, 3 * TILE), _run(rng, 5)])
    tiles = -(-data.size // TILE)
    sizes, odd = pgrammar.tile_sizes(model, data)
    assert tiles > end_tile > 1024 and odd[1024] and odd[1025] and (end_tile < 2048 or (odd[2048] and data.size > 8 << 20))
    assert not model.special[data[start - 1]] and model.special[data[start:start + run.size]].all()
    want = pgrammar.expand(model, data)
    assert want.size == int(sizes.sum())
    print("head scan chunks: %d tiles, %d bytes in, %d bytes out" % (tiles, data.size, want.size))
    _device_case(ctx, g, model, data, want, [(0, 0), (1, 9)], "run to tile %d" % end_tile)
    _block_case(ctx, g, model, data, want, "run to tile %d" % end_tile)


# ---- c. the forms of the offset scan ------------------------------------------------------------------------

@pytest.mark.parametrize("special", [False, True], ids=["plain", "special"])
@pytest.mark.parametrize("n", [4096 * TILE, 4096 * TILE + 1, (64 << 20) + 12345], ids=["4096_tiles", "4097_tiles", "64MiB"])
def test_scan_forms(ctx, n, special):
    """Gap 2: one-workgroup scan up to 4096 tiles, k_scan_reduce + k_scan_apply<true> above.  Random bytes: the
    tiles' totals all differ, so a wrong offset moves bytes."""
    if special:
        kit = pgrammar.special_kit()
    else:
        kit = pgrammar.Kit(keep=pgrammar.PLAIN)
        for m in (2, 3, 5, 17, 33):
            kit.variable(m)
    g, model = _loaded(kit)
    rng = np.random.default_rng(n + special)
    data = _random_bytes(rng, model, n)
    tiles = -(-n // TILE)
    sizes, _ = pgrammar.tile_sizes(model, data)
    assert sizes.size == tiles and (np.diff(sizes) != 0).mean() > 0.9
    want = pgrammar.expand(model, data)
    st = _device_case(ctx, g, model, data, want, [(0, 0), (1, 5)] if n < 32 << 20 else [(8, 11)], "scan %d" % n)
    assert st["launches"] == (3 if special else 1) + (1 if tiles <= 4096 else 2) + 1
    print("scan form: %d tiles, %d launches, %d bytes out, ms_device %.3f" % (tiles, st["launches"], want.size, st["ms_device"]))
    if n < 32 << 20:
        _block_case(ctx, g, model, data, want, "scan %d" % n)


# ---- d. nothing to write --------------------------------------------------------------------------------------

def test_tiles_and_blocks_that_stand_for_nothing(ctx, oracle):
    """Gap 6: tiles whose total is 0 between, before and behind full ones, and a whole block of them."""
    kit, g, model, og = _special(ctx, oracle)
    assert model.of(pgrammar.EMPTY_PAIR) == b""
    rng = np.random.default_rng(44)
    empty = pgrammar.symbols([pgrammar.EMPTY_PAIR] * (TILE // 2))
    full = _plain_filler(rng, kit, TILE)
    for name, parts in (("between", [full, empty, full]), ("first", [empty, full, full]), ("last", [full, full, empty]),
                        ("two between", [full, empty, empty, full[:100]]), ("alternating", [empty, full, empty, full, empty])):
        data = np.concatenate(parts)
        want = _expect(model, data, og, oracle)
        sizes, _ = pgrammar.tile_sizes(model, data)
        assert (sizes == 0).sum() == sum(p is empty for p in parts)
        _device_case(ctx, g, model, data, want, _placements(1 << 20), "empty tile " + name)
        _block_case(ctx, g, model, data, want, "empty tile " + name)
    for tiles in (1, 3):
        data = np.tile(empty, tiles)
        want = _expect(model, data, og, oracle)
        assert want.size == 0
        st = _device_case(ctx, g, model, data, want, [(0, 0), (1, 1), (15, 8)], "empty block")
        assert st["route"] == 1 and st["out_bytes"] == 0 and st["launches"] == 4
        _block_case(ctx, g, model, data, want, "empty block")
    data = pgrammar.symbols([pgrammar.EMPTY_PAIR])
    _device_case(ctx, g, model, data, _expect(model, data, og, oracle), [(0, 0), (3, 5)], "one empty pair")


# ---- e. size limits ---------------------------------------------------------------------------------------------

def test_capacity_bound_switches_the_route(ctx, oracle):
    """Gap 5: cap = 2^32 - 1 is the device's, cap = 2^32 the host function's; same bytes, both entry points.  The
    buffers have the output's real size: a capacity is a bound, and the guards show nothing beyond the output is
    touched."""
    kit, g, model, og = _special(ctx, oracle)
    rng = np.random.default_rng(45)
    data = _random_bytes(rng, model, 3 * TILE + 5)
    want = _expect(model, data, og, oracle)
    for cap, route in (((1 << 32) - 1, 1), (1 << 32, 2), ((1 << 40), 2)):
        _device_case(ctx, g, model, data, want, [(0, 0), (1, 15)], "cap %d" % cap, cap=cap, route=route)
        _block_case(ctx, g, model, data, want, "cap %d" % cap, cap=cap, route=route)


def test_a_tile_that_stands_for_more_than_32_bits(ctx):
    """Gap 5: 4096 tokens of 2^20 + 1 bytes in one tile (k_pp_count's clamp): refused by both entry points, nothing
    written, and the context works on."""
    kit, var, others = pgrammar.length_grammar((1 << 20) + 1)
    g, model = _loaded(kit)
    data = pgrammar.symbols([var] * TILE)
    assert pgrammar.expansion_size(model, data) == (1 << 32) + TILE
    cap = (1 << 32) - 1
    with Arena(ctx, data.size, 1 << 16) as arena:
        n_out, back = arena.run(g, data, cap)
        assert n_out == -1 and (back == FILL).all()
    out = np.full(1 << 16, FILL, np.uint8)
    n = hip._u64(0)
    assert ctx.lib.bwtc_hip_postprocess_block(ctx.handle, g.h, hip._ptr(data), data.size, hip._ptr(out), cap, ctypes.byref(n)) == -1
    assert (out == FILL).all()
    small = pgrammar.symbols([var, pgrammar.PLAIN[0], others[17]])
    want = pgrammar.expand(model, small)
    _device_case(ctx, g, model, small, want, [(0, 0), (1, 1)], "after the refusal")
    _block_case(ctx, g, model, small, want, "after the refusal")


CHUNK = 256 << 20


def _download(ctx, d_ptr, k, buf):
    assert ctx.lib.bwtc_hip_memcpy_to_host(ctx.handle, buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_ptr), k) == 0
    return buf[:k]


def test_outputs_at_the_top_of_32_bits():
    """Gap 5: an output of exactly 2^32 - 1 bytes, and one 3 tokens shorter (not a multiple of 16), from about 2^20
    tokens of 4097 bytes (256 tiles of 16 MiB each) and one closing token; cap equal to the size.  One byte less of
    capacity: refused, nothing written.  Expected bytes in closed form: the token's bytes tiled (the construction
    test_pgrammar.py holds against the model at a small size).  A context of its own: the workspace never shrinks."""
    T = (1 << 32) - 1
    A = 4097
    count = (T - 4200) // A
    rest = T - count * A
    kit = pgrammar.Kit(keep=pgrammar.PLAIN)
    a, b = kit.variable(A), kit.variable(rest)
    g, model = _loaded(kit)
    ea, eb = np.frombuffer(model.of(a), np.uint8), np.frombuffer(model.of(b), np.uint8)
    rep = np.tile(ea, CHUNK // A + 3)
    back = np.empty(CHUNK, np.uint8)
    fill = np.full(CHUNK, FILL, np.uint8)
    with hip.Context(0, 1 << 20) as ctx:
        d_in = ctx.dmalloc(count + 1 + GUARD)
        d_out = ctx.dmalloc(GUARD + T + GUARD)
        out = d_out + GUARD
        try:
            def expected(lo, k, tokens):                      # bytes [lo, lo + k) of `tokens` tokens a, then b
                e = rep[lo % A:lo % A + k].copy()
                edge = tokens * A
                if lo + k > edge:
                    e[max(edge - lo, 0):] = eb[max(lo - edge, 0):lo + k - edge]
                return e

            def compare(tokens, size):
                for lo in range(0, size, CHUNK):
                    k = min(CHUNK, size - lo)
                    got = _download(ctx, out + lo, k, back)
                    _same(got, expected(lo, k, tokens), "bytes from %d" % lo)

            for lo in range(0, GUARD + T + GUARD, CHUNK):
                ctx.to_device(d_out + lo, fill[:min(CHUNK, GUARD + T + GUARD - lo)])
            data = pgrammar.symbols([a] * count + [b])
            ctx.to_device(d_in, np.concatenate([data, np.full(GUARD, FILL, np.uint8)]))
            # one byte less than the block stands for: refused and nothing written
            with pytest.raises(hip.BwtcHipError) as e:
                ctx.postprocess_device(g, d_in, data.size, out, T - 1)
            assert e.value.code == -1
            for lo in range(0, GUARD + T + GUARD, CHUNK):
                k = min(CHUNK, GUARD + T + GUARD - lo)
                assert (_download(ctx, d_out + lo, k, back) == FILL).all(), "a refused block wrote bytes"
            t0 = time.time()
            assert ctx.postprocess_device(g, d_in, data.size, out, T) == T
            st = ctx.postprocess_stats()
            print("2^32 - 1 bytes out: %d tokens in %d tiles, ms_device %.3f, wall %.2f s"
                  % (data.size, -(-data.size // TILE), st["ms_device"], time.time() - t0))
            _check_stats(st, model, data, T)
            compare(count, T)
            assert (ctx.to_host(d_out, GUARD) == FILL).all() and (ctx.to_host(out + T, GUARD) == FILL).all()
            assert (ctx.to_host(d_in + data.size, GUARD) == FILL).all()
            # three tokens fewer: 2^32 - 1 - 3 * 4097 bytes, 12 modulo 16
            T2 = T - 3 * A
            assert T2 % 16 == 12
            data2 = pgrammar.symbols([a] * (count - 3) + [b])
            ctx.to_device(d_in, np.concatenate([data2, np.full(GUARD, FILL, np.uint8)]))
            ctx.to_device(out + T2, fill[:GUARD])
            assert ctx.postprocess_device(g, d_in, data2.size, out, T2) == T2
            _check_stats(ctx.postprocess_stats(), model, data2, T2)
            compare(count - 3, T2)
            assert (ctx.to_host(d_out, GUARD) == FILL).all() and (ctx.to_host(out + T2, GUARD) == FILL).all()
        finally:
            ctx.dfree(d_in)
            ctx.dfree(d_out)


def test_input_sizes_around_2_to_the_31():
    """Gap 5: n = 2^31 - 1 is the device's (route 1), n = 2^31 the host function's (route 2): plain bytes with tokens
    near the start, the middle and the end, the same bytes on both sides.  Input and expected output in closed form
    (a periodic pattern of plain bytes, uploaded and compared in pieces).  bwtc_hip_postprocess_device only: the
    other entry point's host route is covered by test_capacity_bound_switches_the_route."""
    kit = pgrammar.Kit(keep=pgrammar.PLAIN)
    a, b = kit.variable(17), kit.variable(4097)
    g, model = _loaded(kit)
    P = 113
    pattern = (128 + np.arange(P)).astype(np.uint8)
    assert all(len(model.plain[c]) == 1 for c in pattern)
    rep = np.tile(pattern, CHUNK // P + 3)
    back = np.empty(CHUNK, np.uint8)
    with hip.Context(0, 1 << 20) as ctx:
        for n, route in (((1 << 31) - 1, 1), (1 << 31, 2)):
            tokens = {5: a, 6: b, (1 << 30) + 3: b, n - 2: a, n - 1: b}      # input position -> variable
            size = n + sum(len(model.of(v)) - 1 for v in tokens.values())
            d_in = ctx.dmalloc(n + GUARD)
            d_out = ctx.dmalloc(GUARD + size + GUARD)
            out = d_out + GUARD
            try:
                for lo in range(0, n, CHUNK):
                    k = min(CHUNK, n - lo)
                    piece = rep[lo % P:lo % P + k].copy()
                    for at, v in tokens.items():
                        if lo <= at < lo + k:
                            piece[at - lo] = v
                    ctx.to_device(d_in + lo, piece)
                ctx.to_device(d_in + n, np.full(GUARD, FILL, np.uint8))
                ctx.to_device(d_out, np.full(GUARD, FILL, np.uint8))
                ctx.to_device(out + size, np.full(GUARD, FILL, np.uint8))
                t0 = time.time()
                assert ctx.postprocess_device(g, d_in, n, out, size) == size
                st = ctx.postprocess_stats()
                print("n = %d: route %d, ms_device %.3f, wall %.2f s" % (n, st["route"], st["ms_device"], time.time() - t0))
                assert st["route"] == route and st["in_bytes"] == n and st["out_bytes"] == size, st
                if route == 1:
                    assert st["tokens"] == n and st["pair_tokens"] == 0 and st["pool_bytes"] == model.pool_bytes, st
                    assert st["launches"] == 1 + 2 + 1, st
                # the output: stretches of the pattern (by input position) between the tokens' bytes
                at_in = at_out = 0
                for pos in sorted(tokens) + [n]:
                    while at_in < pos:                         # plain bytes [at_in, pos)
                        k = min(CHUNK, pos - at_in)
                        _same(_download(ctx, out + at_out, k, back), rep[at_in % P:at_in % P + k], "plain bytes from input %d" % at_in)
                        at_in += k
                        at_out += k
                    if pos < n:
                        e = np.frombuffer(model.of(tokens[pos]), np.uint8)
                        _same(ctx.to_host(out + at_out, e.size), e, "the token at input %d" % pos)
                        at_in += 1
                        at_out += e.size
                assert at_out == size
                assert (ctx.to_host(d_out, GUARD) == FILL).all() and (ctx.to_host(out + size, GUARD) == FILL).all()
                assert (ctx.to_host(d_in + n, GUARD) == FILL).all()
            finally:
                ctx.dfree(d_in)
                ctx.dfree(d_out)


# ---- f. one context, many calls -----------------------------------------------------------------------------------

def test_one_context_many_calls(oracle):
    """Gap 7: workspace regrowth and reuse, the switch between grammars with and without special symbols, a refusal
    followed by a success, the entry points alternating; the statistics describe the last call only."""
    rng = np.random.default_rng(46)
    sk = pgrammar.special_kit()
    tiny = pgrammar.Kit(keep=pgrammar.PLAIN)
    tiny_var = tiny.variable(2)
    big_kit, big_var, big_others = pgrammar.length_grammar((1 << 20) + 1)
    assert big_kit.model().pool_bytes > 100 * sk.model().pool_bytes > 100 * tiny.model().pool_bytes

    def special_data(n):
        return _random_bytes(rng, sk.model(), n)

    steps = [("special, 2 MiB", sk, special_data(2 << 20), "device"),
             ("tiny, 3 bytes", tiny, pgrammar.symbols([tiny_var, pgrammar.PLAIN[0], tiny_var]), "block"),
             ("no rules", None, rng.integers(0, 256, 70000, dtype=np.uint8), "device"),
             ("no rules, block", None, rng.integers(0, 256, 5, dtype=np.uint8), "block"),
             ("special, refused", sk, special_data(1 << 20), "refuse-device"),
             ("special, 1 MiB", sk, special_data(1 << 20), "block"),
             ("tiny, refused", tiny, pgrammar.symbols([tiny_var] * 9000), "refuse-block"),
             ("tiny, 9000 tokens", tiny, pgrammar.symbols([tiny_var] * 9000), "device"),
             ("special, 6 MiB: larger than any before", sk, special_data(6 << 20), "device"),
             ("large pool after a small one", big_kit, pgrammar.symbols([big_var, big_others[33], big_var]), "block"),
             ("tiny again", tiny, pgrammar.symbols([pgrammar.PLAIN[1], tiny_var]), "device"),
             ("large pool, device", big_kit, pgrammar.long_mix(rng, list(big_others.values()), big_var, (1 << 20) + 1, 300, 4 << 20), "device"),
             ("special, 6 MiB again", sk, special_data(6 << 20), "block"),
             ("special only", sk, _run(rng, 3 * TILE + 1), "device")]
    none = pgrammar.expansions([])
    workspace = 0
    with hip.Context(0, 1 << 20) as ctx:
        for what, kit, data, how in steps:
            g, model = _loaded(kit) if kit else (hip.Grammar(), none)
            want = pgrammar.expand(model, data)
            if how.startswith("refuse"):
                cap = max(want.size - 1, model.min_cap())
                assert cap < want.size
                if how == "refuse-device":
                    with Arena(ctx, data.size, want.size) as arena:
                        n_out, back = arena.run(g, data, cap, 1, 1)
                    assert n_out == -1 and (back == FILL).all(), what
                else:
                    out = np.full(want.size, FILL, np.uint8)
                    n = hip._u64(0)
                    rc = ctx.lib.bwtc_hip_postprocess_block(ctx.handle, g.h, hip._ptr(data), data.size, hip._ptr(out), cap, ctypes.byref(n))
                    assert rc == -1 and (out == FILL).all(), what
                st = ctx.postprocess_stats()
                assert st["in_bytes"] == data.size and st["out_bytes"] == 0, (what, st)
            elif how == "device":
                st = _device_case(ctx, g, model, data, want, [(1, 3), (0, 0)], what)
            else:
                st = _block_case(ctx, g, model, data, want, what)
            assert st["workspace_bytes"] >= workspace, (what, st, workspace)
            workspace = st["workspace_bytes"]
