"""tests/rankmodel.py held to what is independent of it (no GPU): the numpy suffix array against sorted() over byte
strings, every list honest against that suffix array (keys ascending along it), the vectorised ranking step equal to one
written slot by slot in plain Python -- every MODE, every emit form, every initial form, a round -- the two properties
*placed* and *refined* on the model's output of every case, each named case at the edge it is named for, the scan and
key expectations against their own plain restatements, and the whole chain -- initial ranking and every round, each fed
the one before -- ending at the true suffix array and the transform's bytes, and every driver case to its route.  tests/test_gpu_rank_step.py runs the same
cases on the device."""
import numpy as np
import pytest

import rankmodel as rm

CASES = rm.pass_cases()


def _sorted_sa(T):
    b = bytes(np.asarray(T, np.uint8))
    return np.array(sorted(range(len(b)), key=lambda i: b[i:]), np.uint32)


def _same(want, slow, mode):
    return [f for f in rm.compared(mode) if not np.array_equal(np.asarray(want[f], np.uint64), np.asarray(slow[f], np.uint64))]


def _honest(L):
    kc = (L["keys"].astype(np.uint64) & np.uint64(L["kmask"])).astype(object)
    wc = (L["w"].astype(np.int64) & L["long"]["wmask"]) if L["w"] is not None else np.zeros(L["m"], np.int64)
    pairs = list(zip(kc.tolist(), wc.tolist()))
    return all(a <= b for a, b in zip(pairs, pairs[1:]))


def test_suffix_array_against_sorted():
    texts = [c["T"] for name, c in CASES.items() if len(c["T"]) <= 7000] + list(rm.emit_texts().values()) + [rm.bytes_text(3000, 1)]
    for T in texts:
        assert np.array_equal(rm.suffix_array(T), _sorted_sa(T))


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_honest_reaches_its_edge_and_keeps_both_properties(name):
    c = CASES[name]
    T, L = c["T"], rm.make_list(c)
    SA = rm.sa_of(T)
    assert _honest(L), "the keys do not ascend along the suffix array"
    res = rm.expect_pass(T, L, 0, 2, out_n=L["n"] - 1)
    assert rm.edge_holds(c, L, res), "the case does not reach %r" % (c["edge"],)
    assert rm.placed_breaks(T, SA, res, 2, L["n"] - 1) == 0
    assert rm.refined_breaks(T, SA, *rm.left_of(res, 0), L["claim"]) == 0
    if L["m"] <= 9000:
        assert _same(res, rm.slow_pass(T, L, 0, 2, out_n=L["n"] - 1), 0) == []


def test_every_form_mode_and_emit_against_the_slow_pass():
    T0 = rm.form_text(6000, 8)
    SA0 = rm.sa_of(T0)
    CT, cforms = rm.code_forms()
    for fname, (L, e) in list(rm.init_forms(T0).items()) + list(cforms.items()):
        T, SA = (CT, rm.sa_of(CT)) if fname in cforms else (T0, SA0)
        assert _honest(L), fname
        for mode in range(4):
            for emit in (0, e):
                kw = dict(out_n=L["n"] - (mode & 1), lf_n=(0, 5, 256, 2)[mode], rec_shift=3 * mode, plane=mode != 2 or emit != 0)
                res = rm.expect_pass(T, L, mode, emit, **kw)
                assert _same(res, rm.slow_pass(T, L, mode, emit, **kw), mode) == [], (fname, mode, emit)
                assert rm.placed_breaks(T, SA, res, emit, kw["out_n"]) == 0, (fname, mode, emit)
                assert rm.refined_breaks(T, SA, *rm.left_of(res, mode), rm.claimed_depth(L, res)) == 0, (fname, mode, emit)
    T, SA = T0, SA0
    for carry in (False, True):
        L, rank, h = rm.round_list(T, 4, carry)
        assert L["m"] > 2 * rm.TILE and _honest(L)
        assert (np.diff(L["aglob"]) > 1).any(), "aglob has no gaps"
        for mode in range(4):
            for emit in ((0, 2, 1) if carry else (0, 2)):
                res = rm.expect_pass(T, L, mode, emit, lf_n=3)
                assert _same(res, rm.slow_pass(T, L, mode, emit, lf_n=3), mode) == [], (carry, mode, emit)
                assert rm.placed_breaks(T, SA, res, emit) == 0
                assert rm.refined_breaks(T, SA, *rm.left_of(res, mode), 2 * h) == 0
        # a group whose head lies in the tile before: its slot is read through aglob across the seam
        res = rm.expect_pass(T, L, 0, 0)
        seams = np.arange(rm.TILE, L["m"], rm.TILE)
        assert (~res["_head"][seams] & res["_act"][seams]).any()


def test_long_forms_reach_their_fields():
    T = rm.form_text()
    forms = rm.init_forms(T)
    g = forms["gram"][0]
    kc = g["keys"] & np.uint64(g["kmask"])
    wc = g["w"] & np.uint32(g["long"]["wmask"])
    assert ((kc[1:] == kc[:-1]) & (wc[1:] != wc[:-1])).any(), "no items equal in the key and apart in w"
    assert g["long"]["wmask"] < 2 ** 32 - 1 and (g["w"] & ~np.uint32(g["long"]["wmask"])).any()
    lv = forms["levels"][0]
    lvl = ((lv["keys"] >> np.uint64(lv["long"]["lvl_shift"])) & np.uint64(7)).astype(np.int64)
    assert set(lvl[:rm.TILE].tolist()) == set(range(8)), "levels 0..7 are not mixed inside the first tile"
    CT, cforms = rm.code_forms()
    clv = ((cforms["code"][0]["keys"] >> np.uint64(cforms["code"][0]["long"]["lvl_shift"])) & np.uint64(7)).astype(np.int64)
    assert len(set(clv.tolist())) >= 3, "the code keys have fewer than three levels"
    sp = forms["split"][0]
    assert int((sp["keys"] >> np.uint64(48)).max()) == (rm.FORM_TEXT_N - 1) >> 16 >= 1
    # the neighbour across a wave chunk's first slot lies in the other half of an aligned word: odd and even list sizes
    assert rm.FORM_TEXT_N % 2 == 1


def test_emission_cases_reach_their_edges():
    texts = rm.emit_texts()
    T = texts["suffix0_last"]
    L = rm.list_sigma(T, rm.sa_of(T), rm.K)
    res = rm.expect_pass(T, L, 0, 2, out_n=len(T) - 1)
    assert res["pidx"] == len(T) - 1 and res["last_char"] == 0 and res["SA"][len(T) - 1] == 0
    T = texts["suffix0_active"]
    L = rm.list_sigma(T, rm.sa_of(T), rm.K)
    res = rm.expect_pass(T, L, 0, 2)
    assert res["pidx"] == rm.P32 and 0 in res["aidx"][:int(res["counts"][0])]
    xs = []
    for n, lf_n in rm.LF_CASES:
        T = rm.random_text(n, 4, n + lf_n, tail=2)
        res = rm.expect_pass(T, rm.list_sigma(T, rm.sa_of(T), 8), 0, 2, lf_n=lf_n)
        isa = np.argsort(rm.sa_of(T))
        if lf_n > 1:
            x = n // lf_n
            xs.append(x)
            noted = np.flatnonzero(res["lf"] != rm.P32)
            assert all(res["lf"][q] == isa[n - q * x] for q in noted) and (len(noted) == 0 or (noted.min() >= 1 and noted.max() < lf_n))
            assert len(noted) >= (lf_n - 1) // 2 or lf_n < 5, "few of the sampled suffixes are finished"
        else:
            assert (res["lf"] == rm.P32).all()
    assert set(xs) >= {1, 3, 13, 819}
    T = rm.bytes_text(20000, 3)
    L, rank, h = rm.round_list(T, 1, True, wide=True)
    res = rm.expect_pass(T, L, 0, 1)
    fin = ~res["_act"]
    assert len(set((L["keys"][fin] >> np.uint64(56)).tolist())) == 256, "the finished suffixes do not carry all 256 byte values"


def test_scan_expectation_against_a_plain_loop():
    for nt in (1, 257, 4097, 8193):
        for kind in ("zeros", "random", "sum_max", "max_first", "max_part_end"):
            a, b, c = rm.scan_inputs(nt, kind)
            ea, eb, ec, parts, counts = rm.expect_scan(a, b, c)
            sa = sb = mx = 0
            for i in range(nt):
                assert (int(ea[i]), int(eb[i]), int(ec[i])) == (sa & 0xFFFFFFFF, sb & 0xFFFFFFFF, mx), (nt, kind, i)
                sa, sb, mx = sa + int(a[i]), sb + int(b[i]), max(mx, int(c[i]))
            assert (int(counts[0]), int(counts[1])) == (sa & 0xFFFFFFFF, sb & 0xFFFFFFFF)
            assert len(parts) == 3 * -(-nt // rm.SCAN_CHUNK)
            if kind == "sum_max":
                assert sa == 2 ** 32 - 1 and sb == 2 ** 32 - 1


@pytest.mark.parametrize("kind", ["phrases", "runs", "bytes"])
def test_chain_ends_at_the_true_suffix_array(kind):
    T = dict(phrases=rm.form_text(9000, 5), runs=rm.runs_text([40, 9, 2100, 5], tail=7), bytes=rm.bytes_text(6000, 2))[kind]
    n = len(T)
    SA = rm.sa_of(T)
    L0 = rm.list_sigma(T, SA, 1 if kind == "bytes" else 4)
    got_SA, out, pidx, last_char, lf, rounds = rm.chain(T, L0, out_n=n - 1, lf_n=5)
    assert rounds >= 2
    assert np.array_equal(got_SA, SA)
    want = np.where(SA > 0, T[np.maximum(SA.astype(np.int64) - 1, 0)], 0)
    assert np.array_equal(out[:n - 1], want[:n - 1]) and last_char == int(want[n - 1]) and pidx == int(np.flatnonzero(SA == 0)[0])
    isa = np.argsort(SA)
    assert all(lf[q] == isa[n - q * (n // 5)] for q in range(1, 5))


def test_key_expectations():
    """The rounds' keys, spot values worked out by hand."""
    T = np.array([2, 1, 2, 1, 1, 3], np.uint8)
    rank = np.array([3, 1, 4, 0, 2, 5], np.uint32)
    keys = rm.expect_key2(T, [0, 4, 5], [1, 1, 2], rank, [9, 8, 7], 2, 3)
    assert keys.tolist() == [(9 << 56) | (1 << 3) | 5, (8 << 56) | (1 << 3) | 0, (7 << 56) | (2 << 3) | 0]
    text = rm.expect_text(T, [0, 4], [3, 3], None, 1, 3)
    assert text.tolist() == [(3 << 28) | (0x010201 << 4) | 3, (3 << 28) | (0x030000 << 4) | 1]
    k = np.array([1, 1, 1, 2, 1, 1], np.uint32)
    run = rm.expect_key2(T, [3, 0], [0, 0], None, None, 2, 4, run_mode=1, k=k, p=1)
    assert run.tolist() == [(1 << 3) | (6 - 2), 0]         # T[5] = 3 > 1: rising, n - k; k < h and no rank[]: 0
    # T = 2 1 2 1 1 3 3, runs 1 1 1 2 1 2 1.  Suffix 5 (3 3): its run of 2 ends at n, so it is falling and its key is k = 2.
    # Suffix 3 (1 1 3 3): T[5] = 3 > 1, rising: 1 << (b2 - 1) | n - k.  Suffix 2 (k = 1 < h = 2) looks rank[2 + 2] up.
    T7 = np.array([2, 1, 2, 1, 1, 3, 3], np.uint8)
    k7 = np.array([1, 1, 1, 2, 1, 2, 1], np.uint32)
    r7 = np.array([4, 1, 3, 0, 2, 6, 5], np.uint32)
    assert rm.stretch_lengths(T7, 1).tolist() == k7.tolist()
    run = rm.expect_key2(T7, [5, 3, 2], [1, 1, 1], r7, None, 2, 5, run_mode=1, k=k7, p=1)
    assert run.tolist() == [(1 << 5) | 2, (1 << 5) | (1 << 4) | (7 - 2), (1 << 5) | (2 + 1)]
    # mode 2 at h = 1 behind a step at h_split = 2: suffix 3 (k = 2 >= h_split) is looked up at s + max(h, k) = 5, rank 6;
    # suffix 4 (k = 1 < h_split) at s + h = 5 too; at h = 4 suffix 3 looks at 3 + max(4, 2) = 7, past the end: 0
    m2 = rm.expect_key2(T7, [3, 4], [0, 0], r7, None, 1, 4, run_mode=2, k=k7, h_split=2, p=1)
    assert m2.tolist() == [7, 7]
    m2 = rm.expect_key2(T7, [3, 0], [0, 0], r7, None, 4, 4, run_mode=2, k=k7, h_split=2, p=1)
    assert m2.tolist() == [0, 2 + 1]
    # a text round behind the step: suffix 3 (k = 2 >= h_split = 2) reads from s + k + (h - h_split) = 3 + 2 + 1 = 6: "3", one past
    tx = rm.expect_text(T7, [3], [0], None, 3, 2, run_mode=2, k=k7, h_split=2)
    assert tx.tolist() == [(0x0300 << 4) | 1]


@pytest.mark.parametrize("name", sorted(rm.driver_cases()))
def test_driver_case_takes_its_route_and_keeps_both_properties(name):
    c = rm.driver_cases()[name]
    T, L, rank, kw = rm.make_driver(c)
    want = rm.expect_round(T, L, rank, pairs_min=c["pm"](L["m"]), **kw)
    assert want["route"] == c["route"] and (L["m"] >= 3 * rm.TILE or name == "pairs_unsorted")
    if name == "pairs_unsorted":
        assert (len(T) - 1).bit_length() <= 12 < (len(rm.driver_cases()["pairs_sorted"]["T"]) - 1).bit_length()
    if c["route"] == "dense":
        assert 2 * want["m"] >= L["m"]
    if c["route"] == "pairs":
        assert 2 * want["m"] < L["m"]
    SA = rm.sa_of(T)
    assert rm.placed_breaks(T, SA, want["step"], 1 if kw["emit"] else 0, kw["out_n"]) == 0
    assert rm.refined_breaks(T, SA, *rm.round_left(want, want["route"] == "raw"), None) == 0
    if want["route"] != "raw" and want["m"]:                       # the next list is sorted, and a permutation of the active members
        bits = 64 if not want["carry"] else 56
        kk = want["ks"] & np.uint64((1 << bits) - 1) if bits < 64 else want["ks"]
        assert (np.diff(kk.astype(object)) >= 0).all()
        assert np.array_equal(np.sort(want["vs"]), np.sort(L["sfx"][want["step"]["_act"]]))
    if c.get("run_mode") == 1:
        assert want["ran_run"] and (rm.stretch_lengths(T, 1)[want["vs"]] >= kw["h_next"]).any()
