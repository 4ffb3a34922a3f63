"""tests/codemodel.py held to truths it did not restate (no GPU): every built row is prefix free, alphabetic, complete
and at most 26 bits long; the model's keys are monotone along sorted() over the dense-code strings and their levels
never claim more shared characters than there are; the vectorised key maker equals a suffix-by-suffix one made of
Python strings; and every named case of tests/test_gpu_code_keys.py reaches the edge it is named for."""
import numpy as np
import pytest

import codemodel as cm

_MADE = {}


def _made(c):
    """A case's input and the model's answer, made once."""
    if c["name"] not in _MADE:
        inp = cm.make(c)
        _MADE[c["name"]] = (inp, cm.expected(c, inp))
    return _MADE[c["name"]]


_ORDERS = {}


def _order(T, lut):
    key = (T.tobytes(), np.asarray(lut).tobytes())
    if key not in _ORDERS:
        _ORDERS[key] = cm.suffix_order(T, lut)
    return _ORDERS[key]


def test_level_thresholds():
    for level, first in enumerate(cm.LEVEL_MIN):
        assert int(cm.level_of(first)) == level and int(cm.level_depth(level)) == first
        if level:
            assert int(cm.level_of(first - 1)) == level - 1
    assert int(cm.level_of(72)) == 7 and int(cm.level_of(1)) == 0
    assert all(int(cm.level_depth(cm.level_of(k))) <= k for k in range(1, 73))     # a level never claims more than k


def test_dense_codes_keep_the_order():
    rng = np.random.default_rng(5)
    for lone in (False, True):
        for _ in range(20):
            vals = rng.choice(np.arange(1, 256), int(rng.integers(1, 255)), replace=False)
            T = vals[rng.integers(0, vals.size, 500)].astype(np.uint8)
            T[:vals.size] = vals
            T[-1] = 0
            lut, sigma = cm.lut_of(T, lone)
            present = sorted(set(T.tolist()) - ({0} if lone else set()))
            assert sigma == max(2, len(present))
            assert [int(lut[b]) for b in present] == list(range(len(present)))
            assert lut[0] == 0 and all(lut[b] <= lut[b + 1] for b in range(255))
            assert all(int(lut[b]) == 0 for b in range(present[0]))                  # below the smallest present byte
    lut, sigma = cm.lut_of(np.arange(256, dtype=np.uint8), False)
    assert sigma == 256 and (lut == np.arange(256)).all()
    assert cm.lut_of(np.zeros(3, np.uint8), False)[1] == 2 and cm.lut_of(np.zeros(1, np.uint8), True)[1] == 2


def test_pair_counts_against_a_loop():
    rng = np.random.default_rng(6)
    for n in (1, 2, 17, 4096, 4097, 3 * 4096 + 5):
        T = rng.integers(0, 5, n).astype(np.uint8)
        lut, _ = cm.lut_of(T, False)
        want = np.zeros((256, 256), np.int64)
        for j in range(1, n):                       # fewer than 512 tiles: every pair of the text once
            want[lut[T[j - 1]], lut[T[j]]] += 1
        assert np.array_equal(cm.pair_counts(T, lut), want), n
    # above 512 tiles: workgroup b takes tile floor(b * ntiles / 512), no tile twice
    for ntiles in (513, 1500):
        tiles = cm.sampled_tiles(ntiles * 4096 - 9)
        assert len(tiles) == 512 and len(set(tiles)) == 512 and tiles[0] == 0 and tiles == sorted(tiles) and tiles[-1] < ntiles


@pytest.mark.parametrize("bucket", cm.buckets("table"))
def test_adversarial_rows_are_prefix_free_alphabetic_complete_and_short(bucket):
    """The count sets of the GPU test's table cases: every row of the model's table is prefix free, alphabetic (the
    left-aligned codewords strictly increase with the symbol) and complete (Kraft sum exactly 1, in integers; an
    alphabet of one symbol: one codeword of one bit), no codeword is longer than 26 bits, the error word is 0."""
    for c in (c for c in cm.cases("table") if c["bucket"] == bucket):
        inp, exp = _made(c)
        chk = cm.table_checks(exp["table"], c["sigma"])
        assert chk["ok"] and chk["prefix_free"] and chk["alphabetic"] and chk["complete"], (c["name"], chk)
        assert chk["longest"] <= cm.MAX_LEN and exp["err"] == 0, (c["name"], chk["longest"])


def test_deepest_adversarial_codeword():
    """Geometric, Fibonacci and tripling weights with a row total of up to 65535 make the deepest trees: 17 bits in
    the model, far from the 26 the table's entries hold."""
    deepest = max(cm.properties(c, *_made(c))["longest"] for c in cm.cases("table"))
    assert deepest == max(cm.properties(c, *_made(c))["longest"] for c in cm.cases("table") if c["kind"] == "deep")
    assert 16 <= deepest <= cm.MAX_LEN
    print("deepest codeword of the table cases: %d bits" % deepest)


def test_product_tables_of_the_stage_cases():
    for c in cm.cases("stage") + [c for c in cm.cases("counts") if c["n"] <= cm.KEYS_UP_TO]:
        inp, exp = _made(c)
        chk = cm.table_checks(exp["table"], exp["sigma"])
        assert chk["ok"] and chk["prefix_free"] and chk["alphabetic"] and chk["complete"] and chk["longest"] <= cm.MAX_LEN, (c["name"], chk)
        assert exp["err"] == 0


def _keys_by_strings(T, lut, table, kbits, split):
    """make_keys suffix by suffix, the bit strings as Python strings."""
    n = T.size
    code = cm.padded_codes(T, lut).tolist()
    word = lambda row, s: format(int(table[row, s]) & 0x7FFFFFF, "0%db" % (int(table[row, s]) >> 27))
    hi_shift, chr_shift, lvl_shift = cm.key_layout(kbits, split)
    keys, w = [], []
    for i in range(n):
        s = word(256, code[i])
        complete, j = 1, i + 1
        while len(s) < kbits:
            s += word(code[j - 1], code[j])
            complete += len(s) <= kbits
            j += 1
        v = int(s[:kbits], 2)
        level = sum(1 for t in cm.LEVEL_MIN[1:] if complete >= t)
        key = (v >> 32) | ((code[i - 1] if i else 0) << chr_shift) | (level << lvl_shift)
        if split:
            key |= (i >> 16) << hi_shift
        keys.append(key)
        w.append(v & 0xFFFFFFFF)
    return np.array(keys[::-1], np.uint64), np.array(w[::-1], np.uint32)


def test_key_maker_against_strings():
    picked = [c for c in cm.cases("keys") if c["bucket"] in ("levels", "need") or (c["n"] <= 1025 and c["kbits"] in (40, 65, 72))]
    picked += [c for c in cm.cases("counts") if c["n"] <= 4097]
    assert len(picked) > 60
    for c in picked:
        inp, exp = _made(c)
        lut, table = (inp["lut"], inp["table"]) if c["form"] == "keys" else (exp["lut"], exp["table"])
        T = inp["T"]
        got = cm.make_keys(T, lut, table, c["kbits"], c["split"])
        keys, w = _keys_by_strings(T, lut, table, c["kbits"], c["split"])
        assert np.array_equal(got["keys"], keys) and np.array_equal(got["w"], w), c["name"]
        assert np.array_equal(got["plane"], (w & 255).astype(np.uint8))


def _first_principles(c, inp, exp, lut):
    order = _order(inp["T"], lut)
    assert cm.monotone_breaks(order, exp["hi"], exp["lo"]) == 0, c["name"]
    assert cm.level_breaks(order, exp["hi"], exp["lo"], exp["level"], inp["T"], lut) == 0, c["name"]
    # what the device's arrays would be unpacked to is what the model holds
    hi, lo, level = cm.unpack(exp["keys"], exp["w"], c["kbits"], c["split"])
    assert np.array_equal(hi, exp["hi"]) and np.array_equal(lo, exp["lo"]) and np.array_equal(level, exp["level"])


@pytest.mark.parametrize("bucket", cm.buckets("keys"))
def test_monotone_and_level_of_the_key_cases(bucket):
    for c in (c for c in cm.cases("keys") if c["bucket"] == bucket):
        inp, exp = _made(c)
        _first_principles(c, inp, exp, inp["lut"])


@pytest.mark.parametrize("bucket", cm.buckets("stage"))
def test_monotone_and_level_of_the_stage_cases(bucket):
    for c in (c for c in cm.cases("stage") if c["bucket"] == bucket):
        inp, exp = _made(c)
        _first_principles(c, inp, exp, exp["lut"])


def test_monotone_and_level_of_the_count_cases():
    for c in (c for c in cm.cases("counts") if c["want_keys"]):
        inp, exp = _made(c)
        _first_principles(c, inp, exp, exp["lut"])


def test_the_two_properties_notice_a_wrong_key():
    """The checks themselves: a key one too large, and a level one too high, are seen."""
    c = [c for c in cm.cases("stage") if c["kbits"] == 40][0]
    inp, exp = _made(c)
    order = _order(inp["T"], exp["lut"])
    lo = exp["lo"].copy()
    lo[order[len(order) // 2]] += np.uint64(1 << 20)
    hi = exp["hi"].copy()
    hi[order[3]] = hi.max() + np.uint64(1)
    assert cm.monotone_breaks(order, exp["hi"], lo) + cm.monotone_breaks(order, hi, exp["lo"]) >= 1
    level = np.minimum(exp["level"] + 1, 7)
    assert cm.level_breaks(order, exp["hi"], exp["lo"], level, inp["T"], exp["lut"]) > 0


@pytest.mark.parametrize("group", ["counts", "table", "keys", "stage"])
def test_every_case_reaches_its_edge(group):
    for c in cm.cases(group):
        inp, exp = _made(c)
        p = cm.properties(c, inp, exp)
        for name, want in c["edge"].items():
            assert p[name] == want, (c["name"], name, p[name], want)
        if c["form"] == "stage":
            assert p["distinct_tiles"] and p["lone_ok"] and p["merged"] in (None, bool(c["lone"])), c["name"]
        if group != "keys" and c["form"] == "stage" and c["n"] > cm.KEYS_UP_TO:
            _MADE.pop(c["name"])                        # (the 2 - 6 MiB texts)


def test_the_key_cases_cover_every_branch_of_the_bit_cutting():
    below32 = need32 = need64 = above64 = 0
    ks, needs, levels = set(), set(), set()
    for c in cm.cases("keys"):
        p = cm.properties(c, *_made(c))
        below32 += p["below32"]; need32 += p["need32"]; need64 += p["need64"]; above64 += p["above64"]
        ks |= set(p["k"]); needs |= set(p["need"]); levels |= set(p["levels"])
    assert below32 and need32 and need64 and above64
    assert set(range(14, 33)) <= needs and set(range(64, 72)) <= needs
    assert set(cm.LEVEL_TARGETS) <= ks and levels == set(range(8))          # both sides of every level threshold
    mixed = [cm.properties(c, *_made(c)) for c in cm.cases("keys") if c["table"] == "mixed" and c["n"] >= 1023 and c["text"] == "random"]
    assert all(p["offsets"] == 32 and p["straddles"] > 0 and p["longest"] == 26 for p in mixed)
