"""GPU tests of the pair-replacing pre-stage's kernels (bwtc_amd/csrc/prepr.hip) at their limits: the statistics
counter by counter, and single rounds through bwtc_hip_pair_replace_device on the caller's device buffers -- the source
at every offset from 16-byte alignment (pr_load's two paths), the destination guarded -- over the blocks of
tests/prblocks.py, whose premises tests/test_prblocks.py proves on the CPU.  The references are the oracle's
PairReplacer and, for the counters, the numpy restatement of the counting rule as well."""
import numpy as np
import pytest

import prblocks as pb
from bwtc_amd import hip

pytestmark = pytest.mark.gpu
GUARD = 64
LEAD = 256                                                    # bytes before the destination: its front guard


@pytest.fixture(scope="module")
def ctx():
    with hip.Context(0, 8 << 20) as c:
        yield c


class Source:
    """A block in the caller's device memory at `offset` from a 256-byte boundary."""

    def __init__(self, ctx, data, offset=0):
        self.ctx, self.n = ctx, data.size
        self.raw = ctx.dmalloc(offset + data.size + 512)
        self.ptr = (self.raw + 255) // 256 * 256 + offset
        ctx.to_device(self.ptr, data)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.dfree(self.raw)


def _device_stats(ctx, data, offset):
    with Source(ctx, data, offset) as src:
        f, pf = ctx.test_pair_stats(src.ptr, data.size)
        f2, pf2 = ctx.test_pair_stats(src.ptr, data.size)      # the counters are cleared by the step itself
    assert (f == f2).all() and (pf == pf2).all(), "a second call counts differently"
    return f, pf


def _device_round(ctx, grammar, data, src_off=0, dst_off=0, room=None):
    """One round into guarded device memory: (replaced, output bytes).  Asserts that nothing but the output was
    written: the 0xA5 fill is intact before the destination and from the output's end to the end of the guard."""
    n = data.size
    room = 2 * n if room is None else room
    size = LEAD + dst_off + room + GUARD
    raw = ctx.dmalloc(size + 256)
    try:
        base = (raw + 255) // 256 * 256
        ctx.to_device(base, np.full(size, 0xA5, np.uint8))
        with Source(ctx, data, src_off) as src:
            n_out, replaced = ctx.pair_replace_device(grammar, src.ptr, n, base + LEAD + dst_off)
        back = ctx.to_host(base, size)
    finally:
        ctx.dfree(raw)
    at = LEAD + dst_off
    assert n_out <= room
    assert (back[:at] == 0xA5).all(), "the front guard was written"
    assert (back[at + n_out:] == 0xA5).all(), "bytes behind the output were written"
    return replaced, back[at:at + n_out].copy()


def _same_round(ctx, oracle, data, want, src_off=0, dst_off=0):
    """The device round against the oracle's (rep, bytes, grammar bytes); returns the device grammar."""
    rep, w, raw = want
    g = hip.Grammar()
    replaced, got = _device_round(ctx, g, data, src_off, dst_off)
    where = (data.size, src_off, dst_off)
    assert replaced == rep, where
    assert got.size == w.size, where
    assert got.tobytes() == w.tobytes(), (where, np.flatnonzero(got != w)[:4])
    assert g.write().tobytes() == raw.tobytes(), where
    return g, got


def _oracle_round(oracle, data):
    og = oracle.OracleGrammar()
    rep, w = oracle.oracle_pair_replace_round(og, data)
    return rep, w, og.write()


def _expands_back(g, got, data):
    back = g.postprocess(got, data.size + 8)
    assert back.size == data.size and back.tobytes() == data.tobytes()


# ---- 1. the statistics, every counter ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", pb.sizes())
def test_pair_statistics_are_exact(ctx, oracle, n):
    blocks = dict(pb.stat_edges(n, 1))
    for ending in pb.ENDINGS:
        blocks["seams_" + ending] = pb.pairs_on_seams(n, ending)
    for name, data in blocks.items():
        f, pf = oracle.oracle_pair_statistics(data)
        rf, rpf = pb.pair_counts(data)
        assert (f == rf).all() and (pf == rpf).all(), name
        for offset in pb.offsets(n):
            df, dpf = _device_stats(ctx, data, offset)
            assert dpf.size == 65536 and df.size == 256
            bad = np.flatnonzero(dpf != pf)
            assert bad.size == 0, (name, n, offset, [(hex(int(i)), int(dpf[i]), int(pf[i])) for i in bad[:4]])
            assert (dpf == rpf).all() and (df == f).all() and (df == rf).all(), (name, n, offset)


# ---- 2. one round at every alignment ----------------------------------------------------------------------------

def _round_blocks(n):
    blocks = {"seams_" + e: pb.pairs_on_seams(n, e) for e in pb.ENDINGS}
    blocks.update({"runs_" + w: pb.double_runs(n, w) for w in pb.WHERE})
    return blocks


@pytest.mark.parametrize("n", pb.sizes())
def test_one_round_is_exact_at_every_alignment(ctx, oracle, n):
    for name, data in _round_blocks(n).items():
        want = _oracle_round(oracle, data)
        for k, (src_off, dst_off) in enumerate([(o, 0) for o in pb.offsets(n)] + [(0, 1), (0, 7)]):
            g, got = _same_round(ctx, oracle, data, want, src_off, dst_off)
            if k == 0:
                _expands_back(g, got, data)
        if n >= 4094:
            assert want[0] >= 1, name                          # the premise (tests/test_prblocks.py), not taken on trust


# ---- 3. runs over the head scan's chunk of 1024 tiles -----------------------------------------------------------

@pytest.mark.parametrize("name", ["long", "tile1024"])
def test_runs_across_the_head_scans_chunk(ctx, oracle, name):
    data = pb.long_double_run() if name == "long" else pb.run_at_tile_1024()
    assert data.size > 1025 * pb.TILE
    want = _oracle_round(oracle, data)
    assert bytes([pb.X, pb.X]) in pb.replaced_pairs(want[2])
    g, got = _same_round(ctx, oracle, data, want, src_off=1 if name == "long" else 0)
    assert bytes([pb.X, pb.X]) in pb.replaced_pairs(g.write())
    _expands_back(g, got, data)


# ---- 4. one count decides ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("double", [False, True])
def test_one_count_decides(ctx, oracle, double):
    build = pb.one_count_decides_double if double else pb.one_count_decides
    pair = bytes([pb.X, pb.X]) if double else bytes(pb.P)
    for k in (1003, 1004):
        data = build(k)
        want = _oracle_round(oracle, data)
        for src_off in (0, 3):
            g, got = _same_round(ctx, oracle, data, want, src_off)
            assert (pair in pb.replaced_pairs(g.write())) == (k == 1004), (k, src_off)
            assert (g.rules == 1) == (k == 1004)
        with Source(ctx, data, 5) as src:
            _, pf = ctx.test_pair_stats(src.ptr, data.size)
        assert pf[pair[0] << 8 | pair[1]] == k
        _expands_back(g, got, data)


# ---- 5. a tile that writes 8192 bytes ---------------------------------------------------------------------------

def test_a_tile_of_escapes_only(ctx, oracle):
    data = pb.all_escaped_tile()
    want = _oracle_round(oracle, data)
    for src_off in (0, 9):
        g, got = _same_round(ctx, oracle, data, want, src_off)
    special = np.array([g.is_special(c) for c in range(256)])
    assert g.special_symbols == 2 and special.sum() == 2
    assert special[got[:2 * pb.TILE]].all() and not special[got[2 * pb.TILE]]
    start, _, out_len = pb.tokens(g.write(), got)
    assert (out_len[:pb.TILE] == 2).all() and start[pb.TILE] == pb.TILE      # tile 0 wrote exactly the first 8192 bytes
    _expands_back(g, got, data)


# ---- 6. round after round until nothing is left to replace -------------------------------------------------------

def test_rounds_to_exhaustion(ctx, oracle):
    data = pb.rounds_to_exhaustion(1)
    original = data
    g, og = hip.Grammar(), oracle.OracleGrammar()
    productive = 0
    for r in range(pb.ROUNDS_CAP):
        rep, w = oracle.oracle_pair_replace_round(og, data)
        replaced, got = _device_round(ctx, g, data, src_off=r % 16)
        assert replaced == rep and got.size == w.size and got.tobytes() == w.tobytes(), r
        assert g.write().tobytes() == og.write().tobytes(), r
        if rep == 0:
            assert got.tobytes() == data.tobytes()             # the copy route
            break
        productive += 1
        data = w
    else:
        pytest.fail("the rounds do not end")
    assert productive >= 7 and g.special_symbols >= 2
    _expands_back(g, data, original)


# ---- 7. refusals ------------------------------------------------------------------------------------------------

def test_lengths_out_of_range_are_refused(ctx):
    data = np.frombuffer(b"abababab" * 8, np.uint8)
    for n in (2, 1 << 31):
        size = LEAD + 128 + GUARD
        raw = ctx.dmalloc(size + 256)
        try:
            base = (raw + 255) // 256 * 256
            ctx.to_device(base, np.full(size, 0xA5, np.uint8))
            with Source(ctx, data) as src:
                g = hip.Grammar()
                with pytest.raises(hip.BwtcHipError) as e:
                    ctx.pair_replace_device(g, src.ptr, n, base + LEAD)
                assert e.value.code == -1 and g.rules == 0
                with pytest.raises(hip.BwtcHipError) as e:
                    ctx.test_pair_stats(src.ptr, n)
                assert e.value.code == -1
                assert ctx.to_host(src.ptr, data.size).tobytes() == data.tobytes()
            assert (ctx.to_host(base, size) == 0xA5).all()
        finally:
            ctx.dfree(raw)
    # and a good block still goes through afterwards
    with Source(ctx, data) as src:
        f, _ = ctx.test_pair_stats(src.ptr, data.size)
    assert f[ord("a")] == f[ord("b")] == 32
