"""GPU tests of the device postprocessor (postprocess.hip behind bwtc_hip_postprocess_device / _block,
Postprocessor::uncompress, preprocessors/Postprocessor.cpp:62-133): precompressed blocks against the input, the
oracle and the host function; data no precompressor wrote under a real grammar; capacity; grammars without rules;
deep grammars; slices decoded side by side with bwtc_hip_decode_block_H_device; the `uncompress` CLI on its three
routes.  Every library case asserts that the device kernels made the bytes (postprocess_stats()["route"] == 1)."""
import os
import re
import subprocess

import numpy as np
import pytest

from bwtc_amd import hip, synth
from test_host_logic import _prepr_inputs
from test_postprocess_abi import arbitrary_cases, special_grammar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5


@pytest.fixture(scope="module")
def ctx():
    with hip.Context(0, 16 << 20) as c:
        yield c


def _expand_device(ctx, g, data, max_size, guard=4096):
    """postprocess_device into a guarded device buffer: (bytes, the guard region behind cap as it was left)."""
    data = np.ascontiguousarray(data, np.uint8)
    d_in = ctx.dmalloc(max(data.size, 1) + 16)
    d_out = ctx.dmalloc(max_size + guard + 16)
    try:
        if data.size:
            ctx.to_device(d_in, data)
        ctx.to_device(d_out, np.full(max_size + guard, GUARD, np.uint8))
        try:
            n = ctx.postprocess_device(g, d_in, data.size, d_out, max_size)
        except hip.BwtcHipError as e:
            return e.code, ctx.to_host(d_out, max_size + guard)
        assert ctx.postprocess_stats()["route"] == 1
        everything = ctx.to_host(d_out, max_size + guard)
        assert (everything[n:] == GUARD).all(), "bytes written behind the expansion"
        return everything[:n].copy(), everything[max_size:]
    finally:
        ctx.dfree(d_in)
        ctx.dfree(d_out)


def _both(ctx, g, data, max_size):
    """The expansion by both entry points, checked to agree and to come from the device kernels."""
    a = ctx.postprocess(g, data, max_size)
    st = ctx.postprocess_stats()
    assert st["route"] == 1 and st["in_bytes"] == np.asarray(data).size and st["out_bytes"] == a.size, st
    b, _ = _expand_device(ctx, g, data, max_size)
    assert isinstance(b, np.ndarray) and a.size == b.size and (a == b).all()
    return a


@pytest.mark.parametrize("name,data", _prepr_inputs(), ids=[n for n, _ in _prepr_inputs()])
def test_precompressed_blocks_expand_to_the_input(ctx, oracle, name, data):
    for opts in ("p", "pp", "ppppp"):
        g, og = hip.Grammar(), oracle.OracleGrammar()
        pre = ctx.precompress(g, opts, data)
        oracle.oracle_precompress(og, opts, data)
        got = _both(ctx, g, pre, data.size)
        assert got.size == data.size and (got == data).all(), (name, opts)
        want = oracle.oracle_postprocess(og, pre, data.size + 8)
        assert got.size == want.size and (got == want).all(), (name, opts)
        host = g.postprocess(pre, data.size + 8)
        assert got.size == host.size and (got == host).all(), (name, opts)


def test_a_16_MiB_text_block(ctx, oracle):
    """Many tiles, every tile offset non-trivial."""
    data = synth.gen_text(16 << 20, 21)
    g = hip.Grammar()
    pre = ctx.precompress(g, "ppppp", data)
    assert pre.size < 0.6 * data.size
    got = _both(ctx, g, pre, data.size)
    assert got.size == data.size and (got == data).all()
    st = ctx.postprocess_stats()
    assert st["tokens"] == pre.size - st["pair_tokens"] and st["launches"] >= 3 and st["workspace_bytes"] > 0, st


def test_arbitrary_data_under_a_real_grammar(ctx):
    g, _, _ = special_grammar()
    assert g.special_symbols >= 2
    for name, data in arbitrary_cases(g):
        want = g.postprocess(data, 64 * data.size + 64)          # the host function: existing code
        got = _both(ctx, g, data, want.size)
        assert got.size == want.size and (got == want).all(), name
        st = ctx.postprocess_stats()
        assert st["tokens"] + st["pair_tokens"] == data.size, (name, st)     # every byte belongs to one token


def test_capacity_is_exact_and_a_refused_block_writes_nothing(ctx):
    g, pre, data = special_grammar()
    for block, size in ((pre, data.size),):
        got, behind = _expand_device(ctx, g, block, size)
        assert isinstance(got, np.ndarray) and got.tobytes() == data.tobytes() and (behind == GUARD).all()
        assert ctx.postprocess(g, block, size).tobytes() == data.tobytes()
        # one byte less: the host function's error, and nothing written
        with pytest.raises(hip.BwtcHipError) as host_err:
            g.postprocess(block, size - 1)
        code, everything = _expand_device(ctx, g, block, size - 1)
        assert code == host_err.value.code == -1
        assert (everything == GUARD).all()
        out = np.full(size, GUARD, np.uint8)
        n = hip._u64(0)
        rc = ctx.lib.bwtc_hip_postprocess_block(ctx.handle, g.h, hip._ptr(block), block.size, hip._ptr(out), size - 1, hip.ctypes.byref(n))
        assert rc == -1 and (out == GUARD).all()
    # many tiles: the total is what is checked, not a tile's share
    text = synth.gen_text(1 << 20, 5)
    g2 = hip.Grammar()
    pre2 = ctx.precompress(g2, "ppppp", text)
    code, everything = _expand_device(ctx, g2, pre2, text.size - 1)
    assert code == -1 and (everything == GUARD).all()
    got, behind = _expand_device(ctx, g2, pre2, text.size)
    assert got.tobytes() == text.tobytes() and (behind == GUARD).all()


def test_a_grammar_without_rules_copies(ctx):
    g = hip.Grammar()
    for n in (0, 1, 2, 3, 5000):
        data = (np.arange(n) % 251).astype(np.uint8)
        got, behind = _expand_device(ctx, g, data, max(n, 1))
        assert isinstance(got, np.ndarray) and got.tobytes() == data.tobytes() and (behind == GUARD).all()
    code, everything = _expand_device(ctx, g, np.zeros(10, np.uint8), 9)
    assert code == -1 and (everything == GUARD).all()


def test_tiny_blocks_under_a_grammar_with_rules(ctx):
    g, _, _ = special_grammar()
    special = [c for c in range(256) if g.is_special(c)][0]
    plain = [c for c in range(256) if not g.is_special(c)][0]
    for data in ([], [plain], [special], [plain, special], [special, special], [special, plain, special], [plain, plain, plain]):
        data = np.array(data, np.uint8)
        want = g.postprocess(data, 1 << 16)
        got, behind = _expand_device(ctx, g, data, 1 << 16)
        assert isinstance(got, np.ndarray) and got.tobytes() == want.tobytes(), data


def _deepest_variable(g):
    """The byte whose expansion under g is longest (and not a special symbol)."""
    best, size = None, 0
    for c in range(256):
        if g.is_special(c):
            continue
        n = g.postprocess(np.array([c], np.uint8), 1 << 20).size
        if n > size:
            best, size = c, n
    return best, size


def test_deep_grammars(ctx):
    for data in (np.frombuffer(b"ab" * 2 ** 18, np.uint8),
                 np.frombuffer(b"0123456789abcdefghijklmnopqrstuv" * 40000, np.uint8)):
        g = hip.Grammar()
        pre = ctx.precompress(g, "ppppp", data)
        got = _both(ctx, g, pre, data.size)
        assert got.size == data.size and (got == data).all()
        var, size = _deepest_variable(g)
        assert size >= 32, size                                     # five rounds: expansions of 32 bytes
        # token-dense: the same grammar fed one of its deepest variables a million times
        dense = np.full(1_000_000, var, np.uint8)
        want = g.postprocess(dense, size * dense.size)
        assert want.size == size * dense.size
        got = _both(ctx, g, dense, want.size)
        assert got.size == want.size and (got == want).all()


def test_slices_cut_inside_a_pair_expand_in_one_call(ctx):
    """A precompressed block cut right behind a special byte that starts a pair: the two slices are decoded side by
    side into one device buffer and expanded in one call (a per-slice postprocess would get the cut pair wrong)."""
    g, pre, data = special_grammar()
    cut, i = None, 0
    while i < pre.size:
        if g.is_special(pre[i]) and i + 1 < pre.size:
            if i > 8:
                cut = i + 1
                break
            i += 2
        else:
            i += 1
    if cut is None:
        pytest.skip("the grammar's precompressed block has no pair that starts with a special symbol")
    records = [ctx.transform_and_encode(part, 8)[0] for part in (pre[:cut], pre[cut:])]
    room = 2 * data.size + 64
    d_pre = ctx.dmalloc(room)
    d_out = ctx.dmalloc(data.size + 16)
    try:
        used = 0
        for rec in records:
            size, consumed = ctx.decode_block_H_device(rec, d_pre + used, room - used)
            assert consumed == rec.size
            assert ctx.huffman_decode_stats()["route"] == 1
            used += size
        assert used == pre.size and (ctx.to_host(d_pre, used) == pre).all()
        n = ctx.postprocess_device(g, d_pre, used, d_out, data.size)
        assert ctx.postprocess_stats()["route"] == 1
        assert n == data.size and (ctx.to_host(d_out, n) == data).all()
        # what a per-slice postprocess makes of it differs
        apart = np.concatenate([g.postprocess(pre[:cut], 4 * data.size), g.postprocess(pre[cut:], 4 * data.size)])
        assert apart.tobytes() != data.tobytes()
    finally:
        ctx.dfree(d_pre)
        ctx.dfree(d_out)


def _tally(stderr):
    m = re.search(r"^postprocess: device (\d+) host (\d+) ms_device ([0-9.]+)$", stderr, re.M)
    assert m, stderr
    return int(m.group(1)), int(m.group(2)), float(m.group(3))


@pytest.mark.parametrize("coder", ["H", "B"])
def test_uncompress_cli_postprocesses_on_the_device(tmp_path, coder):
    exe = os.path.join(ROOT, "bwtc_amd", "host", "compress")
    unexe = os.path.join(ROOT, "bwtc_amd", "host", "uncompress")
    assert os.path.exists(exe) and os.path.exists(unexe)
    data = np.concatenate([synth.gen_text(1_600_000, 3), synth.gen_random_bytes(50_000, 1), np.zeros(20_000, np.uint8),
                           synth.gen_text(700_000, 4)])
    src, dst = tmp_path / "input.bin", tmp_path / "input.bwtc"
    src.write_bytes(data.tobytes())
    # --mem 1: precompressor blocks of 740 000 bytes
    r = subprocess.run([exe, "-m", "1", "-s", "8", "-e", coder, "--prepr", "ppppp", str(src), str(dst)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(name, **env):
        out = tmp_path / name
        r = subprocess.run([unexe, str(dst), str(out)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, BWTC_HIP_DEBUG="1", **env))
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == data.tobytes(), name
        return _tally(r.stderr)

    device, host, ms = run("default.bin")
    assert device > 0 and host == 0 and ms > 0, (device, host, ms)
    device, host, _ = run("post_host.bin", BWTC_HIP_POSTPROCESS="host")
    assert device == 0 and host > 0, (device, host)
    run("decode_host.bin", BWTC_HIP_DECODE="host")
    # nothing new is printed without the switch
    env = {k: v for k, v in os.environ.items() if k != "BWTC_HIP_DEBUG"}
    r = subprocess.run([unexe, str(dst), str(tmp_path / "quiet.bin")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "postprocess:" not in r.stderr
