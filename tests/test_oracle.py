"""CPU tests: the oracle (oracle/bwtc_oracle.c) against the golden vectors generated from
the reference's libdivsufsort, the reference's own known-answer asserts, the golden stream
recorded from the reference's Compressor, and (when present) the reference build itself."""
import base64
import hashlib
import json
import os

import numpy as np
import pytest

import blockgen
from bwtc_amd import synth

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    with open(os.path.join(G, name)) as f:
        return json.load(f)


def test_oracle_matches_small_goldens(oracle):
    cases = _load("bwt_small.json")["cases"]
    assert len(cases) >= 50
    for c in cases:
        data = np.frombuffer(base64.b64decode(c["input"]), np.uint8)
        bwt, lf, freqs = oracle.oracle_bwt_block(data, c["sp"])
        assert bwt.tobytes() == base64.b64decode(c["bwt"]), c["name"]
        assert [int(x) for x in lf] == c["lf"], c["name"]
        want = np.zeros(256, np.uint32)
        for k, v in c["freqs_nonzero"].items():
            want[int(k)] = v
        assert (freqs == want).all(), c["name"]
        rc, inv = oracle.oracle_inverse_bwt_block(bwt, lf)
        assert rc == 0 and inv.tobytes() == data.tobytes(), c["name"]


def test_oracle_matches_large_golden_1mib(oracle):
    c = [x for x in _load("bwt_large.json")["cases"] if x["name"] == "C1_random_1MiB"][0]
    d = getattr(synth, c["gen"])(c["size"], c["seed"])
    assert hashlib.sha256(d.tobytes()).hexdigest() == c["input_sha256"]
    bwt, lf, _ = oracle.oracle_bwt_block(d, c["sp"])
    assert hashlib.sha256(bwt.tobytes()).hexdigest() == c["bwt_sha256"]
    assert [int(x) for x in lf] == c["lf"]


def test_generators_are_stable():
    for c in _load("bwt_large.json")["cases"]:
        if c["size"] > (4 << 20):
            continue
        d = getattr(synth, c["gen"])(c["size"], c["seed"])
        assert hashlib.sha256(d.tobytes()).hexdigest() == c["input_sha256"], c["name"]


def test_oracle_vs_reference_build_random(oracle):
    """400 small seeded blocks: the oracle gives the reference's answers, as stored in
    tests/golden/bwt_ref_random.json, and those of the reference build itself where oracle/_ref
    was built."""
    cases = _load("bwt_ref_random.json")["cases"]
    sweep = list(blockgen.reference_sweep())
    assert len(cases) == len(sweep) == 400
    for i, (c, (d, sp)) in enumerate(zip(cases, sweep)):
        assert (d.size, sp, blockgen.digest(d)) == (c["size"], c["sp"], c["input"]), ("input", i)
        a = oracle.oracle_bwt_block(d, sp)
        assert [blockgen.digest(x) for x in a] == [c["bwt"], c["lf"], c["freqs"]], i
        if oracle.ref() is not None:
            b = oracle.ref_bwt_block(d, sp)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all(), i


def test_suffix_array_is_sorted(oracle):
    # the property test/SaisTest.cpp:55-70 checks: SA sorted, SA[0] == size for 0-terminated input
    rng = np.random.default_rng(3)
    for _ in range(10):
        n = int(rng.integers(2, 400))
        t = np.concatenate([rng.integers(0, 4, n).astype(np.uint8), [0]]).astype(np.uint8)
        sa = oracle.oracle_suffix_array(t)
        assert sa[0] == n
        b = t.tobytes()
        suf = [b[i:] for i in sa]
        assert suf == sorted(suf)


def test_reference_known_answers(oracle):
    import ctypes
    ka = _load("utils_known_answers.json")
    L = oracle.lib()
    for c in ka["run_frequencies"]:
        src = np.frombuffer(c["input"].encode(), np.uint8)
        rf = np.zeros(256, np.uint64)
        L.orc_run_frequencies(oracle._ptr(rf), oracle._ptr(src), src.size)
        want = np.zeros(256, np.uint64)
        for k, v in c["expect"].items():
            want[ord(k)] = v
        assert (rf == want).all(), c["ref"]
    for v in ka["packed_integers"]["values"]:
        nb = ctypes.c_int(0)
        p = L.orc_pack_integer(v, ctypes.byref(nb))
        raw = [(p >> (8 * i)) & 0xFF for i in range(nb.value)]
        back = 0
        for i, b in enumerate(raw):
            back |= (b & 0x7F) << (7 * i)
            assert bool(b & 0x80) == (i + 1 < len(raw))
        assert back == v
    for c in ka["huffman_lengths"]:
        fr = np.zeros(256, np.uint64)
        for k, v in c["freqs"].items():
            fr[ord(k)] = v
        cl = np.zeros(256, np.uint32)
        L.orc_huffman_lengths(oracle._ptr(fr), oracle._ptr(cl))
        order = sorted(c["freqs"].items(), key=lambda kv: (kv[1], ord(kv[0])))
        assert [int(cl[ord(k)]) for k, _ in order] == c["sorted_lengths"], c["ref"]
        for k, v in c.get("by_symbol", {}).items():
            assert cl[ord(k)] == v
    bits = np.zeros(64, np.uint8)
    for n, lo, hi, want in ka["binary_code"]["cases"]:
        nb = L.orc_binary_code(n, lo, hi, oracle._ptr(bits))
        assert "".join(str(int(b)) for b in bits[:nb]) == want, (n, lo, hi)


def test_golden_stream_H(oracle):
    c = [x for x in _load("streams.json")["cases"] if x["coder"] == "H"][0]
    s = oracle.oracle_compress_H(c["input_ascii"].encode(), c["block_size"], c["sp"])
    assert s.tobytes() == bytes.fromhex(c["stream_hex"])
    assert oracle.oracle_decompress_H(s, 64).tobytes() == c["input_ascii"].encode()


def test_compress_roundtrip_like_reference_test(oracle):
    # test/CompressorAndDecompressorTest.cpp:61-205: random and repetitive data, single and
    # multiple blocks, 1..30 starting points, coder 'H'.
    rng = np.random.default_rng(11)
    for size, block, sp in [(100, 100, 1), (1000, 300, 3), (100000, 100000, 8), (100000, 18500, 30),
                            (50000, 7000, 2)]:
        for rep in (False, True):
            d = rng.integers(0, 256, size).astype(np.uint8)
            if rep:
                d = np.tile(d[:size // 50 + 1], 51)[:size]
            s = oracle.oracle_compress_H(d, block, sp)
            r = oracle.oracle_decompress_H(s, size + 8)
            assert r is not None and r.tobytes() == d.tobytes()


def test_runs_and_characters_known_answers(oracle):
    # the run counts of test/UtilsTest.cpp:79-129 hold for calculateRunsAndCharacters too
    ka = _load("utils_known_answers.json")
    for c in ka["run_frequencies"]:
        rf, runs, dist = oracle.oracle_runs_and_characters(np.frombuffer(c["input"].encode(), np.uint8))
        for k, v in c["expect"].items():
            assert rf[ord(k)] == v
        assert runs == sum(c["expect"].values()) == sum(dist.values())
        assert sum(l * n for l, n in dist.items()) == len(c["input"])
    rf, runs, dist = oracle.oracle_runs_and_characters(np.frombuffer(b"abdbcarraaa", np.uint8))
    assert runs == 8 and dist == {1: 6, 2: 1, 3: 1}


def _bits(arr, n):
    return "".join(str(int(b)) for b in arr[:n])


def test_wavelet_known_answers(oracle):
    """test/WaveletTest.cpp's known answers against the oracle's restatements: MinimumHeap,
    createHuffmanShape + collectCodes, gammaCode; and the two things the hot path shares with
    them -- the symbol code LENGTHS of the WaveletTree constructor equal the shapes' depths, and
    fixedIntegerCode with W = 0 is the gamma code (WaveletTree.hpp:512)."""
    ka = _load("wavelet_known_answers.json")
    L = oracle.lib()
    for c in ka["heap"]:
        vals = np.array([v for v, _ in c["inserts"]], np.int32)
        wts = np.array([w for _, w in c["inserts"]], np.uint64)
        out = np.zeros(vals.size, np.int32)
        L.orc_min_heap_order(oracle._ptr(vals), oracle._ptr(wts), vals.size, oracle._ptr(out))
        assert out.tolist() == c["delete_order"], c["ref"]
    for c in ka["huffman_shape"]:
        fr = np.zeros(256, np.uint64)
        if "freqs" in c:
            for k, v in c["freqs"].items():
                fr[ord(k)] = v
        else:
            src = np.frombuffer(c["run_string"].encode(), np.uint8)
            L.orc_run_frequencies(oracle._ptr(fr), oracle._ptr(src), src.size)
        syms = np.zeros(256, np.uint32)
        deps = np.zeros(256, np.uint32)
        bits = np.zeros(64 * 256, np.uint8)
        clen = np.zeros(256, np.uint32)
        n = L.orc_create_huffman_shape(oracle._ptr(fr), oracle._ptr(syms), oracle._ptr(deps),
                                       oracle._ptr(bits), oracle._ptr(clen))
        assert "".join(chr(s) for s in syms[:n]) == c["leaves"], c["ref"]
        assert deps[:n].tolist() == c["depths"], c["ref"]
        for k, code in c["codes"].items():
            assert _bits(bits[64 * ord(k):], clen[ord(k)]) == code, c["ref"]
        # the constructor's own codes (canonical, longest rightmost): same depth per symbol
        bits2 = np.zeros(64 * 256, np.uint8)
        clen2 = np.zeros(256, np.uint32)
        L.orc_wavelet_symbol_codes(oracle._ptr(fr), oracle._ptr(bits2), oracle._ptr(clen2))
        for s, d in zip(c["leaves"], c["depths"]):
            assert clen2[ord(s)] == d, c["ref"]
        # prefix-free and complete (Kraft sum 1) unless there is a single symbol
        if n > 1:
            assert sum(2.0 ** -int(clen2[ord(s)]) for s in c["leaves"]) == 1.0
    bits = np.zeros(128, np.uint8)
    for x, want in ka["gamma_codes"]["cases"]:
        assert _bits(bits, L.orc_gamma_code(x, oracle._ptr(bits))) == want
        assert _bits(bits, L.orc_fixed_integer_code(x, 0, oracle._ptr(bits))) == want


def _wavelet_strings():
    ka = _load("wavelet_known_answers.json")["whole_construction"]
    out = [s.encode() for s in ka["strings"]]
    c7 = ka["construction7"]
    out.append(b"abc" * c7["abc_repeats"] + c7["tail"].encode())
    return out


def test_oracle_wavelet_decoder_round_trips(oracle):
    """The oracle's literal decoder (readShape / decodeTreeBF / message / BitDecoder) against
    the oracle's literal encoder: test/WaveletTest.cpp's WholeConstruction inputs, and the
    matrix of test/CompressorAndDecompressorTest.cpp:61-160 (sizes 100..100 000, repetitions
    0 / 2 / 50, one and several blocks, 1..30 starting points), all three wavelet letters."""
    for s in _wavelet_strings():
        d = np.frombuffer(s, np.uint8)
        for sp in (1, 8):
            st = oracle.oracle_compress_B(d, d.size, sp)
            back = oracle.oracle_decompress_wavelet(st, d.size + 8)
            assert back is not None and back.tobytes() == s
    rng = np.random.default_rng(2024)

    def make(length, reps):
        if reps == 0:
            return rng.integers(0, 256, length, dtype=np.uint8)
        return np.tile(rng.integers(0, 256, length // reps, dtype=np.uint8), reps)

    cases = []
    for length in (100, 1000, 10000, 100000):
        for reps in (0, 2, 50):
            cases.append((length, reps, int(length * 100 * 0.185), 1))      # single block
            cases.append((length, reps, max(int(length * (10 if reps != 2 else 1) * 0.185), 18), 1))
    for sp in range(1, 31):
        cases.append((10000, 0, int(100000 * 0.185), sp))
    for length, reps, block, sp in cases:
        d = make(length, reps)
        for letter in ("B",) if sp > 1 else ("B", "b", "u"):
            st = oracle.oracle_compress_wavelet(letter, d, block, sp)
            back, bwt = oracle.oracle_decompress_wavelet(st, d.size + 8, want_bwt=True)
            assert back is not None and back.tobytes() == d.tobytes(), (length, reps, block, sp, letter)
    # the reference-recorded 36-byte stream decodes to its input
    for c in _load("streams.json")["cases"]:
        if c["coder"] == "B":
            st = np.frombuffer(bytes.fromhex(c["stream_hex"].replace(" ", "")), np.uint8)
            back, bwt = oracle.oracle_decompress_wavelet(st, 64, want_bwt=True)
            assert back.tobytes() == c["input_ascii"].encode() and bwt.tobytes() == b"abdbcarraaa"


def test_oracle_wavelet_decoder_rejects_damage(oracle):
    d = np.frombuffer(b"abracadabra" * 50, np.uint8)
    st = oracle.oracle_compress_B(d, d.size, 1)
    assert oracle.oracle_decompress_wavelet(st, d.size + 8).tobytes() == d.tobytes()
    assert oracle.oracle_decompress_wavelet(st[: st.size // 2], d.size + 8) is None


# ---- pair-replacing pre-stage: the known answers of the reference's own tests ---------------------------
def _prepr_input(case):
    parts = [np.frombuffer((case["repeat"] * case["times"]).encode(), np.uint8)]
    for f in case["fill"]:
        sweep = np.array([c for c in range(256) if chr(c) not in f["skip"]], np.uint8)
        parts += [sweep] * f["times"]
    parts.append(np.frombuffer(case["tail"].encode(), np.uint8))
    return np.concatenate(parts)


def _prepr_cases():
    with open(os.path.join(os.path.dirname(__file__), "golden", "prepr_known_answers.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", _prepr_cases()["pair_replacer"], ids=lambda c: c["name"])
def test_pair_replacer_known_answers(oracle, case):
    """test/PairReplacerTest.cpp: replacements decided, size of the replaced text, special symbols and rules of
    the grammar; and the grammar's serialised form read back expands the text to the input."""
    data = _prepr_input(case)
    g = oracle.OracleGrammar()
    cur = data
    for k, rnd in enumerate(case["rounds"]):
        if rnd.get("first_byte_not_special_before"):
            assert not g.is_special(cur[0])
        rep, cur = oracle.oracle_pair_replace_round(g, cur)
        if rnd["rep"] is not None:
            assert rep == rnd["rep"], (case["name"], k)
        if rnd["size"] is not None:
            assert cur.size == rnd["size"], (case["name"], k)
    if case["specials"] is not None:
        assert g.specials == case["specials"]
    if case["rules"] is not None:
        assert g.rules == case["rules"]
    raw = g.write()
    g2 = oracle.OracleGrammar()
    assert g2.read(raw) == raw.size
    assert (g2.frequencies() == g.frequencies()).all()
    back = oracle.oracle_postprocess(g2, cur, data.size + 16)
    assert back is not None and back.size == data.size and (back == data).all()


def test_grammar_known_answers(oracle):
    """test/GrammarTest.cpp: the empty grammar, and two freed symbols over two new special symbols."""
    ka = _prepr_cases()["grammar"]
    g = oracle.OracleGrammar()
    raw = g.write()
    assert raw.tolist() == [0]
    g2 = oracle.OracleGrammar()
    assert g2.read(raw) == 1 and g2.rules == 0 and g2.specials == 0
    sp = ka["special_symbols"]
    g = oracle.OracleGrammar()
    L = oracle.lib()
    L.orc_grammar_add_rule(g.h, ord(sp["rule"][0]), ord(sp["rule"][1]), ord(sp["rule"][2]))
    freed = np.frombuffer(sp["freed"].encode(), np.uint8)
    spec = np.frombuffer(sp["specials"].encode(), np.uint8)
    pairs = np.zeros(8, np.uint16)
    n = L.orc_grammar_expand_alphabet(g.h, oracle._ptr(freed), freed.size, oracle._ptr(spec), spec.size, oracle._ptr(pairs))
    assert n == len(sp["next_pairs"])
    for k, (a, b) in enumerate(sp["next_pairs"]):
        assert (int(pairs[k]) >> 8, int(pairs[k]) & 0xFF) == (ord(a), ord(b))
    assert g.rules == sp["rules"] and g.specials == sp["n_specials"]
    raw = g.write()
    g2 = oracle.OracleGrammar()
    assert g2.read(raw) == raw.size and g2.rules == g.rules and g2.specials == g.specials


@pytest.mark.parametrize("coder", ["H", "B"])
@pytest.mark.parametrize("prep", ["", "p", "pp", "ppppp"])
def test_prepr_streams_round_trip_in_the_oracle(oracle, coder, prep):
    """The matrix of test/CompressorAndDecompressorTest.cpp:61-205 with the pre-stage on: the oracle's own
    encoder against its own (independent) decoders, several precompressor blocks and slices."""
    rng = np.random.default_rng(17 + len(prep))
    words = [bytes(rng.integers(97, 105, rng.integers(2, 7)).astype(np.uint8)) for _ in range(40)]
    text = b" ".join(words[int(i)] for i in rng.integers(0, 40, 12000))
    for data, mem in ((np.frombuffer(text, np.uint8), 40000), (np.frombuffer(text[:3000], np.uint8), 100000),
                      (rng.integers(0, 256, 5000).astype(np.uint8), 9000)):
        stream = oracle.oracle_compress_prepr(coder, prep, data, mem)
        back = oracle.oracle_decompress_H(stream, data.size + 64) if coder == "H" else oracle.oracle_decompress_wavelet(stream, data.size + 64)
        assert back is not None and back.size == data.size and (back == data).all(), (coder, prep, mem)
