"""CPU tests of tests/pgrammar.py, the test-side grammar writer and expansion model, against the project's host
code and the oracle: the model agrees with both on every grammar a precompressor made of _prepr_inputs(), and both
read, re-write and expand the hand-built grammars of test_gpu_postprocess_limits.py as the model says -- through the
host function and through the kernels' host twin at tiles of 16, 64 and 4096 bytes.  Everything here stays below
MEDIUM = 48 MiB of output; the larger cases of the GPU file have the model (checked here at a small size of the same
construction) as their reference."""
import numpy as np
import pytest

import pgrammar
from test_host_logic import _prepr_inputs

TILES = (16, 64, 4096)
MEDIUM = 48 << 20


@pytest.mark.parametrize("name,data", _prepr_inputs(), ids=[n for n, _ in _prepr_inputs()])
def test_model_agrees_with_the_oracle_on_precompressed_blocks(oracle, name, data):
    from bwtc_amd import hip
    for opts in ("p", "pp", "ppppp"):
        g, og = hip.Grammar(), oracle.OracleGrammar()
        pre = g.host_precompress(opts, data)
        assert oracle.oracle_precompress(og, opts, data).tobytes() == pre.tobytes()
        raw = g.write()
        assert raw.tobytes() == og.write().tobytes()
        rules, specials, freed, used = pgrammar.read(raw)
        assert used == raw.size and len(rules) == g.rules and len(specials) == g.special_symbols
        assert pgrammar.build(rules, specials, freed).tobytes() == raw.tobytes(), (name, opts)
        model = pgrammar.expansions(rules, specials, freed)
        want = oracle.oracle_postprocess(og, pre, data.size + 8)
        got = pgrammar.expand(model, pre)
        assert got.tobytes() == want.tobytes() == data.tobytes(), (name, opts)
        tokens, pairs = pgrammar.token_counts(model, pre)
        assert tokens + pairs == pre.size


def _inputs(name, kit, model):
    """Small and medium inputs under a hand-built grammar: what the GPU file feeds it, at sizes the CPU suite affords."""
    rng = np.random.default_rng(len(name))
    variables = list(kit.length)
    singles = [v for v in variables if not isinstance(v, tuple)]
    out = [("each_alone_%d" % i, pgrammar.symbols([v])) for i, v in enumerate(variables)]
    out.append(("between_plain", pgrammar.symbols([pgrammar.PLAIN[0]] + variables + [pgrammar.PLAIN[1]])))
    short = [v for v in variables if kit.length[v] <= 4097] + list(pgrammar.PLAIN)
    for n in (4095, 4096, 4097, 8193):
        out.append(("mix_%d" % n, pgrammar.mix(rng, short, n)[:n]))
    long_ones = [v for v in singles if kit.length[v] > 4097]
    if long_ones:
        out.append(("long_mix", pgrammar.long_mix(rng, short, long_ones[0], kit.length[long_ones[0]])))
    if kit.specials:
        sp = np.array(kit.specials, np.uint8)
        for k in (4095, 4096, 4097, 3 * 4096 + 1):
            run = sp[rng.integers(0, sp.size, k)]
            out.append(("run_%d" % k, np.concatenate([pgrammar.symbols(pgrammar.PLAIN), run, pgrammar.symbols(singles[:1]), run[:k // 2]])))
            out.append(("only_run_%d" % k, run))
        out.append(("empty_pairs", pgrammar.symbols([pgrammar.EMPTY_PAIR] * 3000)))
        out.append(("random", rng.integers(0, 256, 1 << 18).astype(np.uint8)))
    return out


@pytest.mark.parametrize("name", sorted(pgrammar.small_grammars()))
def test_hand_built_grammars(oracle, name):
    from bwtc_amd import hip
    kit = pgrammar.small_grammars()[name]
    raw, model = kit.grammar(), kit.model()
    g, og = hip.Grammar(), oracle.OracleGrammar()
    assert g.read(raw) == raw.size and og.read(raw) == raw.size
    assert g.write().tobytes() == raw.tobytes() and og.write().tobytes() == raw.tobytes()
    assert g.rules == og.rules == model.n_rules and g.special_symbols == og.specials == len(model.specials)
    for c in range(256):
        assert g.is_special(c) == og.is_special(c) == bool(model.special[c])
    rules, specials, freed, used = pgrammar.read(raw)
    assert used == raw.size and (rules, specials, freed) == (kit.rules, kit.specials, kit.freed)
    for case, data in _inputs(name, kit, model):
        want = pgrammar.expand(model, data)
        assert want.size == pgrammar.expansion_size(model, data) <= MEDIUM, (case, want.size)
        cap = max(want.size, model.min_cap())
        got = oracle.oracle_postprocess(og, data, cap + 8)
        assert got is not None and got.tobytes() == want.tobytes(), case
        assert g.postprocess(data, cap).tobytes() == want.tobytes(), case
        for tile in TILES:
            assert g.host_postprocess_tiles(data, cap, tile).tobytes() == want.tobytes(), (case, tile)
        sizes, _ = pgrammar.tile_sizes(model, data)
        assert int(sizes.sum()) == want.size


def test_build_refuses_what_the_format_cannot_say():
    for rules, specials, freed in (([(1, b"a")], (), ()),                         # a right side of one byte
                                   ([(1, b"abcde")], (), ()),
                                   ([((5, 6), b"ab")], (5,), ()),                  # a pair with a byte that is not special
                                   ([((5, 5), b"ab")], (5,), ()),                  # a double
                                   ([(5, b"ab")], (5,), ()),                       # a special symbol as a variable
                                   ([(1, b"ab")], (5,), (9,)),                     # one special symbol has no pair to give away
                                   ([], (5,), ())):
        with pytest.raises(AssertionError):
            pgrammar.build(rules, specials, freed)
    assert pgrammar.build([]).tobytes() == b"\0"
    assert pgrammar.read(b"\0") == ([], [], [], 1)


def test_periodic_closed_forms_match_the_model():
    """The GiB-sized GPU cases take their expected bytes from np.tile of one token's bytes: the same construction
    at a small size against expand()."""
    kit = pgrammar.Kit(keep=pgrammar.PLAIN)
    a, b = kit.variable(4097), kit.variable(5000)
    model = kit.model()
    data = pgrammar.symbols([a] * 700 + [b])
    want = np.concatenate([np.tile(np.frombuffer(model.of(a), np.uint8), 700), np.frombuffer(model.of(b), np.uint8)])
    assert pgrammar.expand(model, data, piece=1 << 16).tobytes() == want.tobytes()
    assert pgrammar.token_counts(model, data) == (701, 0)
