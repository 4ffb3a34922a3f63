"""The coders 'b' and 'u' with their adaptive models on the GPU (BWTC_HIP_LETTER_MODELS=1, read when a context is
made): the records are the oracle's, with the switch and without, and the route counters say which route made them --
under the switch every block's models ran on the device and were used, without it none did."""
import os
import re
import subprocess

import numpy as np
import pytest

import blockgen
from bwtc_amd import hip, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bwtc_amd", "host", "compress")
UNEXE = os.path.join(ROOT, "bwtc_amd", "host", "uncompress")
LF = np.zeros(1, np.uint32)
LETTERS = ("b", "u")
CTX_BYTES = 5 << 20


def _context(switch, **env):
    """A context made with BWTC_HIP_LETTER_MODELS set to `switch` (None: unset) and `env`; the environment is put back."""
    want = dict(env, BWTC_HIP_LETTER_MODELS=switch)
    old = {k: os.environ.get(k) for k in want}
    try:
        for k, v in want.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return hip.Context(0, CTX_BYTES)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def on():
    with _context("1") as c:
        yield c


@pytest.fixture(scope="module")
def off():
    with _context(None) as c:
        yield c


def _packed(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _frame(coder, records, sizes):
    s = coder.encode()
    for rec, n in zip(records, sizes):
        s += _packed(n) + _packed(1) + b"\x00" + bytes(rec)
    return s + b"\x00"


def _run_heavy(n, seed):
    rng = np.random.default_rng(seed)
    k = n // 20
    return np.repeat(rng.integers(0, 12, k).astype(np.uint8), rng.geometric(1.0 / 40, k))[:n]


def _single_blocks():
    rng = np.random.default_rng(3)
    return [("text", synth.gen_text(300_000, 11)), ("dna", synth.gen_dna(200_000, 12)),
            ("random", rng.integers(0, 256, 100_000).astype(np.uint8)), ("all_equal", np.full(100_000, 7, np.uint8)),
            ("run_heavy", _run_heavy(200_000, 13)), ("64KiB_plus_1", synth.gen_text((64 << 10) + 1, 14))]


SINGLE = _single_blocks()


def _assert_on_device(r, blocks):
    assert r["models_device"] == blocks and r["models_rejected"] == 0 and r["lost_turn"] == 0, r
    assert r["trees_device"] == blocks and r["trees_host"] == 0, r


@pytest.mark.parametrize("letter", LETTERS)
@pytest.mark.parametrize("which", range(len(SINGLE)), ids=[n for n, _ in SINGLE])
def test_single_blocks(which, letter, on, off, oracle):
    name, data = SINGLE[which]
    bwt, lf, freqs = oracle.oracle_bwt_block(data, 8)
    want = oracle.oracle_wavelet_encode_block_with(letter, bwt, lf, freqs).tobytes()
    got = {}
    for ctx in (on, off):
        ctx.wavelet_start(letter)
        ctx.wavelet_routes(reset=True)
        got[ctx] = ctx.wavelet_encode(bwt, lf, freqs, threads=4).tobytes()
        assert got[ctx] == want, (name, letter, ctx is on)
    assert got[on] == got[off]
    # the switch context ran this block's models on the device and used them; the other one did not
    _assert_on_device(on.wavelet_routes(), 1)
    r = off.wavelet_routes()
    assert r["models_device"] == 0 and r["models_rejected"] == 0 and r["trees_device"] == 1, r


def _begin(ctx, blk):
    d_in = ctx.dmalloc(blk.size + 16)
    try:
        ctx.to_device(d_in, blk)
        lf, freqs = ctx.bwt_block_device(d_in, d_in, blk.size, 8)
        out = np.zeros(ctx.compress_bound(blk.size), np.uint8)
        return ctx.wavelet_encode_device_begin(d_in, blk.size, lf, freqs, out, threads=4), out
    finally:
        ctx.dfree(d_in)


def test_letter_changes_with_blocks_under_way(on, oracle):
    """B -> b -> u -> B over nine blocks of 200 KB through _begin / _end with three under way: a block keeps the
    letter it was begun under, and each letter's part is the oracle's stream for it."""
    bs = 200_000
    d = np.concatenate([synth.gen_text(5 * bs, 31), synth.gen_dna(2 * bs, 32), synth.gen_text(2 * bs, 33)])
    blocks = [d[o:o + bs] for o in range(0, d.size, bs)]
    letters = ["B", "B", "b", "b", "b", "u", "u", "B", "B"]
    assert len(blocks) == len(letters) == 9
    on.wavelet_routes(reset=True)
    records, pend, cur = [None] * 9, [], None
    try:
        for i, (blk, letter) in enumerate(zip(blocks, letters)):
            if letter != cur:
                on.wavelet_start(letter)                    # with up to three blocks of the stream before under way
                cur = letter
            pend.append((i,) + _begin(on, blk))
            if len(pend) == 3:
                j, t, out = pend.pop(0)
                records[j] = out[:on.wavelet_encode_end(t)].tobytes()
        for j, t, out in pend:
            records[j] = out[:on.wavelet_encode_end(t)].tobytes()
    finally:
        on.wavelet_reset()
    for a, z in ((0, 2), (2, 5), (5, 7), (7, 9)):
        want = oracle.oracle_compress_wavelet(letters[a], d[a * bs:z * bs], bs, 8).tobytes()
        assert _frame(letters[a], records[a:z], [bs] * (z - a)) == want, (a, z, letters[a])
    _assert_on_device(on.wavelet_routes(), 9)


def test_farm_flow_over_two_contexts(oracle):
    """_prepare / _queue as a caller that farms a 'b' stream over two contexts uses them: each block is queued before
    its context prepares another, so every block's passes keep their turn in the workspace."""
    bs = 1 << 20
    d = np.concatenate([synth.gen_text(3 * bs, 41), synth.gen_dna(bs, 42)])
    blocks = [d[o:o + bs] for o in range(0, d.size, bs)]
    ctxs = [_context("1"), _context("1")]
    try:
        for c in ctxs:
            c.wavelet_start("b")
        state, pend = 4, []
        for i, blk in enumerate(blocks):
            c = ctxs[i % 2]
            d_in = c.dmalloc(blk.size + 16)
            try:
                c.to_device(d_in, blk)
                lf, freqs = c.bwt_block_device(d_in, d_in, blk.size, 8)
                out = np.zeros(c.compress_bound(blk.size), np.uint8)
                t = c.wavelet_encode_device_prepare(d_in, blk.size, lf, freqs, out, threads=4)
            finally:
                c.dfree(d_in)
            state = c.wavelet_encode_queue(t, state)
            assert state == 3                              # what a 'b' block hands on: the state its tasks start from
            pend.append((c, t, out))
        records = [out[:c.wavelet_encode_end(t)].tobytes() for c, t, out in pend]
        assert _frame("b", records, [bs] * len(blocks)) == oracle.oracle_compress_wavelet("b", d, bs, 8).tobytes()
        for k, c in enumerate(ctxs):
            _assert_on_device(c.wavelet_routes(), len(blocks[k::2]))
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("letter", LETTERS)
@pytest.mark.parametrize("override", ["host", "fallback"])
def test_overrides_win_over_the_switch(override, letter, oracle):
    """BWTC_HIP_MODELS=host keeps the models on the worker threads whatever the switch says; under
    BWTC_HIP_TEST_MODELS_FALLBACK=1 a letter's device passes run and are turned down, as a 'B' block's are."""
    bs = 300_000
    d = np.concatenate([synth.gen_text(2 * bs, 51), synth.gen_dna(bs, 52)])
    env = {"BWTC_HIP_MODELS": "host"} if override == "host" else {}
    ctx = _context("1", **env)
    try:
        if override == "fallback":
            os.environ["BWTC_HIP_TEST_MODELS_FALLBACK"] = "1"          # read block by block
        ctx.wavelet_start(letter)
        pend = [_begin(ctx, d[o:o + bs]) for o in range(0, d.size, bs)]
        records = [out[:ctx.wavelet_encode_end(t)].tobytes() for t, out in pend]
        r = ctx.wavelet_routes()
    finally:
        os.environ.pop("BWTC_HIP_TEST_MODELS_FALLBACK", None)
        ctx.close()
    assert _frame(letter, records, [bs] * 3) == oracle.oracle_compress_wavelet(letter, d, bs, 8).tobytes()
    assert r["trees_device"] == 3 and r["models_device"] == 0, r
    if override == "host":
        assert r["models_rejected"] == 0, r
    else:
        assert r["models_rejected"] == 3 and r["reject_reasons"] == hip.REJECT_TEST, r


# the limit blocks of at most 4 MiB -- of blockgen.LIMIT_CASE_NAMES that is sections_inside_runs alone, the others hold
# 24 M bytes and more -- and many_ids, 4.1 MiB: the one with more ids than the dense layout takes
SMALL_LIMITS = ["sections_inside_runs", "many_ids"]


@pytest.mark.parametrize("letter", LETTERS)
@pytest.mark.parametrize("name", SMALL_LIMITS)
def test_limit_cases_under_the_switch(name, letter, on, oracle):
    assert name in blockgen.LIMIT_CASE_NAMES
    [(_, block, _)] = list(blockgen.limit_blocks(names=(name,)))
    assert block.size <= CTX_BYTES
    freqs = np.bincount(block, minlength=256).astype(np.uint32)
    try:
        on.wavelet_start(letter)
        on.wavelet_routes(reset=True)
        got = on.wavelet_encode(block, LF, freqs, threads=4)
        assert got.tobytes() == oracle.oracle_wavelet_encode_block_with(letter, block, LF, freqs).tobytes(), (name, letter)
        _assert_on_device(on.wavelet_routes(), 1)
    finally:
        on.wavelet_reset()


@pytest.mark.parametrize("letter", LETTERS)
def test_cli_with_the_switch(letter, tmp_path, oracle):
    """`compress -e b|u -m 1` on 2 MB under the switch: the oracle's stream, the debug routes line shows the models on
    the device, and `uncompress` gives the input back."""
    assert os.path.exists(EXE) and os.path.exists(UNEXE)
    data = np.concatenate([synth.gen_text(1_700_000, 61), synth.gen_dna(300_000, 62)])
    src, dst, back = tmp_path / "in.bin", tmp_path / "in.bwtc", tmp_path / "back.bin"
    src.write_bytes(data.tobytes())
    env = dict(os.environ, BWTC_HIP_LETTER_MODELS="1", BWTC_HIP_DEBUG="1")
    r = subprocess.run([EXE, "-m", "1", "-s", "8", "-e", letter, str(src), str(dst)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"^bwtc_hip routes: .*$", r.stderr, re.M)
    assert m, r.stderr[-2000:]
    routes = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", m.group(0))}
    assert routes["models_device"] > 0 and routes["models_device"] == routes["trees_device"] and routes["models_rejected"] == 0, routes
    bs = int(1 * 1000000 * 0.185)                          # what -m 1 gives: eleven blocks
    want = oracle.oracle_compress_wavelet(letter, data, bs, 8)
    assert dst.read_bytes() == want.tobytes()
    r = subprocess.run([UNEXE, str(dst), str(back)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and back.read_bytes() == data.tobytes(), r.stderr[-2000:]
