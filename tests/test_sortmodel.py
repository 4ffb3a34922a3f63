"""CPU tests of tests/sortmodel.py, the model tests/test_gpu_sort_limits.py holds the GPU radix sorts to: against
Python's sorted() on item tuples for each of the three forms, the pass plan of the long sort against the order it
must produce, and every named case against the edge it is named for."""
import numpy as np
import pytest

import sortmodel as sm


def _py(a):
    return [int(v) for v in a]


# ---- the model against brute force -------------------------------------------------------------------------------
@pytest.mark.parametrize("ktype", ["u32", "u64"])
def test_plain_model_equals_sorted(ktype):
    W = sm.WIDTH[ktype]
    rng = np.random.default_rng(W)
    ones = (1 << W) - 1
    for bit_lo, nbits, holes in ((0, W, 0), (0, 1, 0), (0, 13, 0), (12, 28, 0), (W - 24, W, 0), (0, 9, 50), (8, 24, 313), (0, 0, 77), (5, 5, 3)):
        n = 400
        k = rng.integers(0, 64, n, dtype=np.uint64) * np.uint64(0x0421084210842109) & np.uint64(ones)    # few values, every bit used
        k = k.astype(sm.DT[ktype])
        if holes:
            full = np.full(n + holes, ones, k.dtype)
            full[np.sort(rng.permutation(n + holes)[:n])] = k
            k = full
        v = rng.integers(0, 1 << 32, k.size, dtype=np.uint64).astype(np.uint32)
        # brute force: the digits the passes take, least significant first, over tuples (stable by construction)
        p = sm.passes(bit_lo, nbits, holes > 0)
        items = [(int(x), int(y), i) for i, (x, y) in enumerate(zip(k, v)) if not (holes and int(x) == ones)]
        if len(items) > 1 or holes:
            for j in range(p):
                items = sorted(items, key=lambda it: (it[0] >> (bit_lo + 8 * j)) & 255)
        # and in one go: by the covered field
        end = min(W, bit_lo + 8 * p)
        assert items == sorted(items, key=lambda it: ((it[0] >> bit_lo) & ((1 << (end - bit_lo)) - 1), it[2])) or len(items) <= 1
        gk, gv = sm.plain_expected(k, v, holes, bit_lo, nbits, "given", "u32")
        assert _py(gk) == [it[0] for it in items] and _py(gv) == [it[1] for it in items], (bit_lo, nbits, holes)
        gk16, gv16 = sm.plain_expected(k, v.astype(np.uint16), holes, bit_lo, nbits, "given", "u16")
        assert _py(gv16) == [it[1] & 0xFFFF for it in items]
        if not holes and nbits > bit_lo:
            m = len(items)
            assert _py(sm.plain_expected(k, None, 0, bit_lo, nbits, "positions")[1]) == [it[2] for it in items]
            assert _py(sm.plain_expected(k, None, 0, bit_lo, nbits, "descending")[1]) == [m - 1 - it[2] for it in items]
            assert _py(sm.plain_expected(k, None, 0, bit_lo, nbits, "descending", "u16")[1]) == [(m - 1 - it[2]) & 0xFFFF for it in items]
            assert sm.plain_expected(k, None, 0, bit_lo, nbits, "keys")[1] is None
    one = np.array([5], sm.DT[ktype])
    assert _py(sm.plain_expected(one, np.array([9], np.uint32))[1]) == [9]          # n = 1: no pass


@pytest.mark.parametrize("kbits,wbits", sm.LONG_BITS + ((5, 11), (8, 8), (12, 3), (64, 1), (2, 31)))
def test_long_model_equals_sorted_and_its_pass_plan(kbits, wbits):
    rng = np.random.default_rng(100 * kbits + wbits)
    n = 500
    k = sm._bits(rng, n, min(kbits, 4)) * np.uint64(0x9E3779B97F4A7C15) & sm._mask(kbits)
    k |= sm._shl(sm._bits(rng, n, 64 - kbits), kbits)
    w = (sm._bits(rng, n, min(wbits, 4)) * np.uint64(0x9E3779B97F4A7C15) & sm._mask(wbits)).astype(np.uint32)
    items = [(int(a), int(b), i) for i, (a, b) in enumerate(zip(k, w))]
    want = sorted(items, key=lambda it: (((it[0] & ((1 << kbits) - 1)) << wbits) | it[1], it[2]))
    gk, gv, gw = sm.long_expected(k, w, kbits, wbits, "u32")
    assert _py(gk) == [it[0] for it in want] and _py(gw) == [it[1] for it in want]
    assert _py(gv) == [n - 1 - it[2] for it in want]
    assert _py(sm.long_expected(k, w, kbits, wbits, "u16")[1]) == [(n - 1 - it[2]) & 0xFFFF for it in want]
    # the plan: ceil((kbits + wbits) / 8) passes whose digits, concatenated, are exactly the order's bits
    plan = sm.long_plan(kbits, wbits)
    assert len(plan) == -(-(kbits + wbits) // 8)
    assert sum(p["bits"] for p in plan) == kbits + wbits and all(1 <= p["bits"] <= 8 for p in plan)
    assert [p["src"] for p in plan] == sorted((p["src"] for p in plan), key=("w", "bridge", "key").index)
    assert sum(p["src"] == "bridge" for p in plan) == (1 if wbits % 8 else 0)
    for p in plan:
        if p["src"] == "bridge":
            assert p["r"] == wbits % 8 and p["shift"] == wbits - p["r"]
    assert (sm.long_order_by_passes(k, w, kbits, wbits) == sm.long_order(k, w, kbits, wbits)).all()
    # by tuples too: pass by pass
    it2 = list(items)
    for p in plan:
        d = sm.long_digit(p, np.array([it[0] for it in it2], np.uint64), np.array([it[1] for it in it2], np.uint32))
        it2 = [it for _, it in sorted(zip(_py(d), it2), key=lambda t: t[0])]
    assert it2 == want


def test_segmented_model_equals_sorted():
    rng = np.random.default_rng(3)
    T = sm.TILE["u32"]
    for bit_lo in (0, sm.STEP_LEAF_SHIFT, 16):
        tf = np.array([0, 0, 1, 1, 3, 3], np.uint32)
        k = (rng.integers(0, 300, 3 * T, dtype=np.uint64) * np.uint64(0x9E3779B1) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        k[T - 40:T] = 0xFFFFFFFF
        k[3 * T - 7:] = 0xFFFFFFFF
        got = sm.seg_expected(k, bit_lo, tf)
        want = []
        for s in range(5):
            seg = [(int(x), i) for i, x in enumerate(k[int(tf[s]) * T:int(tf[s + 1]) * T])]
            want += [x for x, _ in sorted(seg, key=lambda it: ((it[0] >> bit_lo) & 0xFFFF, it[1]))]
        assert _py(got) == want
        assert (got[T - 40:T] == 0xFFFFFFFF).all() and (got[3 * T - 7:] == 0xFFFFFFFF).all()     # the padding stays put


# ---- every named case at its edge ----------------------------------------------------------------------------------
def test_case_list_covers_what_the_gpu_file_promises():
    cs = sm.cases()
    assert len({c["name"] for c in cs}) == len(cs)
    for ktype in ("u32", "u64"):
        T = sm.TILE[ktype]
        seams = [c for c in cs if c["group"] == "seams" and c["ktype"] == ktype]
        want_n = set(sm.SEAM_SMALL) | {t * T + d for t in sm.SEAM_TILES for d in (-1, 0, 1)}
        assert {c["n"] for c in seams} == want_n
        for n in want_n:
            assert {(c["planes"], c["nbits"]) for c in seams if c["n"] == n} == {(p, b) for p in (0, 1) for b in sm.SEAM_NBITS[ktype]}
        dig = [c for c in cs if c["group"] == "digits" and c["ktype"] == ktype]
        assert {(c["shape"], c["n"], c["planes"]) for c in dig} == {(s, n, p) for s in sm.SHAPES for n in (T + 1, 9 * T - 1) for p in (0, 1)}
        holes = [c for c in cs if c["group"] == "holes" and c["ktype"] == ktype]
        for n in (T - 1, T + 1, 2 * T + 1, 9 * T - 1):
            assert {c["n_holes"] for c in holes if c["n"] == n and c["nbits"]} >= {1, T - 1, T, n}
        assert {c["layout"] for c in holes} == {"end", "random", "one_tile", "whole_tile", "alternate"}
        assert any(c["n"] == 1 for c in holes) and any(c["nbits"] == 0 for c in holes)
        assert {c["planes"] for c in holes} == {0, 1}
        vals = [c for c in cs if c["group"] == "values" and c["ktype"] == ktype]
        assert {(c["values"], c["vtype"]) for c in vals} == {("positions", "u32"), ("descending", "u32"), ("keys", "u32"), ("given", "u16"),
                                                             ("descending", "u16")}
        assert {c["n"] for c in vals} == {t * T + d for t in (1, 2, 9) for d in (-1, 1)}
    pay = [c for c in cs if c["group"] == "payload"]
    assert {c["nbits"] for c in pay if c["bucket"] == "u64-bits56_63"} == {40, 48, 56}
    assert {c["bit_lo"] for c in pay} >= {8, 12, 32, 40}
    assert any(c["bit_lo"] > 32 and c["planes"] == 2 for c in pay)                   # the window partition's shape, plane ready
    lg = [c for c in cs if c["form"] == "long"]
    for vtype, el in sm.LONG_INSTS:
        mine = [c for c in lg if (c["vtype"], c["el"]) == (vtype, el)]
        T = sm.LONG_TILE[el]
        assert {(c["kbits"], c["wbits"], c["direct_w"]) for c in mine} == {(k, w, d) for k, w in sm.LONG_BITS for d in (0, 1)}
        assert {c["n"] for c in mine if not c["few"]} == {t * T + d for t in sm.LONG_TILES for d in (-1, 1)}
        assert any(c["few"] for c in mine)
    assert max(c["n"] for c in lg) < 140000 and max(c["n"] + c["n_holes"] for c in cs if c["form"] == "plain") < 150000
    sg = [c for c in cs if c["form"] == "seg"]
    assert {len(c["seg_tiles"]) for c in sg} >= {1, 2, 256} and {c["bit_lo"] for c in sg} == {0, sm.STEP_LEAF_SHIFT}
    assert {t for c in sg for t in c["seg_tiles"]} >= {0, 1, 2, 9}


@pytest.mark.parametrize("group", ["seams", "digits", "payload", "values", "holes", "long", "seg"])
def test_every_named_case_reaches_its_edge(group):
    cs = sm.cases(group)
    assert cs
    for c in cs:
        inp = sm.make(c)
        again = sm.make(c)
        assert all((inp[k] == again[k]).all() for k in inp), c["name"]               # the same input every time
        props = sm.properties(c, inp)
        assert c["edge"], c["name"]
        for key, want in c["edge"].items():
            assert props[key] == want, (c["name"], key, props[key], want)
        if c["form"] == "plain":
            k = inp["keys"]
            W = sm.WIDTH[c["ktype"]]
            assert k.size == c["n"] + c["n_holes"] and k.dtype == sm.DT[c["ktype"]]
            assert int((k == sm._ones(k.dtype)).sum()) == c["n_holes"] or not c["n_holes"]   # without holes it is an item
            # bits from nbits up to the passes' boundary are zero: the covered field is the asked-for field
            end = sm.boundary(c["bit_lo"], c["nbits"], W, c["n_holes"] > 0)
            live = k[k != sm._ones(k.dtype)] if c["n_holes"] else k
            if c["shape"] != "allones":
                assert not (sm._shr(live, c["nbits"]) & sm._mask(end - c["nbits"])).any(), c["name"]
        elif c["form"] == "long":
            assert props["w_fits"] and inp["keys"].size == c["n"] == inp["w"].size
            assert props["has_ties"] or c["n"] < 2 * sm.LONG_TILE[c["el"]], c["name"]
        else:
            assert props["payload_varies"] and props["seg_tiles"] == c["seg_tiles"]


def test_long_cases_name_the_edges_of_the_pass_plan():
    """(40, 32) has no bridge; (33, 21) a bridge of 5 bits of w; (17, 7) and (9, 4) start with the bridge; (3, 4) and (1, 1)
    are one masked digit; (64, 32) leaves no payload room."""
    plan = {kw: sm.long_plan(*kw) for kw in sm.LONG_BITS}
    assert [p["src"] for p in plan[(40, 32)]] == ["w"] * 4 + ["key"] * 5
    assert [(p["src"], p["r"]) for p in plan[(33, 21)]][:3] == [("w", 0), ("w", 0), ("bridge", 5)] and len(plan[(33, 21)]) == 7
    assert plan[(17, 7)][0] == dict(src="bridge", shift=0, bits=8, r=7) and plan[(17, 7)][1]["shift"] == 1
    assert plan[(9, 4)][0] == dict(src="bridge", shift=0, bits=8, r=4) and plan[(9, 4)][1] == dict(src="key", shift=4, bits=5, r=0)
    assert plan[(3, 4)] == [dict(src="bridge", shift=0, bits=7, r=4)]
    assert plan[(1, 1)] == [dict(src="bridge", shift=0, bits=2, r=1)]
    assert len(plan[(64, 32)]) == 12 and plan[(64, 32)][-1] == dict(src="key", shift=56, bits=8, r=0)
    assert [p["src"] for p in plan[(48, 16)]] == ["w"] * 2 + ["key"] * 6
