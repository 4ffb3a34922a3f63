"""tests/finmodel.py held to sorted() (no GPU): the numpy suffix array against sorted() over byte strings, the inputs of
every named case honest against that suffix array, the vectorised model of a pass against one written with sorted()
group by group, the two properties *placed* and *refined* on the model's output of every case, and each family of
named cases at the edge it is named for.  tests/test_gpu_finisher.py runs the same cases on the device."""
import numpy as np
import pytest

import finmodel as fm

CASES = fm.cases()


def _by(prefix):
    return [c for c in CASES if c["bucket"].startswith(prefix)]


def _sorted_sa(T):
    b = bytes(np.asarray(T, np.uint8))
    return np.array(sorted(range(len(b)), key=lambda i: b[i:]), np.uint32)


def test_suffix_array_against_sorted():
    r = np.random.RandomState(5)
    texts = [np.zeros(1, np.uint8), np.array([7, 7], np.uint8), np.zeros(300, np.uint8), fm.ab_text(301, 0), fm.ab_text(300, 17),
             r.randint(0, 2, 5000).astype(np.uint8), r.randint(0, 256, 3000).astype(np.uint8), fm.phrase_text(20000, 3)]
    for T in texts:
        assert np.array_equal(fm.suffix_array(T), _sorted_sa(T))


@pytest.mark.parametrize("bucket", fm.buckets())
def test_cases_are_honest_and_the_model_keeps_both_properties(bucket):
    """Every case: the text's suffix array equals sorted() (texts of at most 20 000 bytes; larger ones: 3000 random
    neighbours compared as byte strings), the list is honest, and the model's output is placed and refined."""
    seen = set()
    for c in _by(bucket):
        if c["bucket"] != bucket:
            continue
        inp = fm.make(c)
        T, SA = inp["T"], inp["SA"]
        if id(T) not in seen:
            seen.add(id(T))
            if len(T) <= 20000:
                assert np.array_equal(SA, _sorted_sa(T)), c["name"]
            else:
                b = bytes(T)
                for k in np.random.RandomState(len(T)).randint(1, len(T), 3000):
                    assert b[int(SA[k - 1]):] < b[int(SA[k]):], (c["name"], int(k))
                assert np.array_equal(np.sort(SA), np.arange(len(T)))
        assert fm.list_breaks(T, SA, inp["regions"], inp["S"], inp["P"], inp["H"], inp["C"]) == 0, c["name"]
        res = fm.run_model(c, inp)
        assert fm.placed_breaks(res, SA) == 0, c["name"]
        assert fm.refined_breaks(T, SA, res) == 0, c["name"]
        m = sum(cnt for _, cnt in inp["regions"])
        finals = int((res["SA"] != fm.POISON).sum())
        assert finals + int(res["next_count"][:16].sum()) + res["hard_count"][0] + res["shallow_count"][0] == m, c["name"]


@pytest.mark.parametrize("bucket", [b for b in fm.buckets() if not b.startswith(("dealing", "rank"))])
def test_vector_model_against_sorted_group_by_group(bucket):
    for c in _by(bucket):
        if c["bucket"] != bucket:
            continue
        inp = fm.make(c)
        want = fm.slow_pass(inp["T"], inp["regions"], inp["S"], inp["P"], inp["H"], inp["C"], **inp["args"])
        have = fm.as_sets(fm.run_model(c, inp))
        assert have[0] == want[0], c["name"]
        assert have[1] == want[1], c["name"]
        assert have[2] == want[2] and have[3] == want[3], c["name"]


def _groups(inp):
    """(region, start in the region, size, depth) of every group."""
    out = []
    for r, (b, cnt) in enumerate(inp["regions"]):
        h = inp["H"][b:b + cnt]
        i = 0
        while i < cnt:
            j = i
            while j + 1 < cnt and h[j + 1] == h[i]:
                j += 1
            out.append((r, i, j - i + 1, int(inp["C"][b + i]) >> 8))
            i = j + 1
    return out


def test_seam_cases_sit_on_their_seams():
    for win, G in fm.SHAPES:
        st = win - G
        cs = {c["name"].split("-", 3)[3]: c for c in _by("seams-%d-%d" % (win, G))}
        for m in (1, 2, st - 1, st, st + 1, win - 1, win, win + 1, 2 * st - 1, 2 * st + 1):
            assert fm.make(cs["list%d" % m])["regions"] == [(cs["list%d" % m]["seed"] % 5, m)]
        sizes = [g[2] for g in _groups(fm.make(cs["sizes"]))]
        for g in (1, 2, G - 1, G, G + 1, 2 * G, win + 1, 3 * st + 5):
            assert g in sizes
        for a in (0, 1, st - 1, st, st + 1, 2 * st - 1, 2 * st, 2 * st + 1):
            for g in (2, G, G + 1):
                assert (0, a, g) in [x[:3] for x in _groups(fm.make(cs["start%d_g%d" % (a, g)]))]
        gs = _groups(fm.make(cs["first_last_owned"]))
        assert gs[0][2] == G and gs[-1][2] == G
        gs = _groups(fm.make(cs["first_last_hard"]))
        assert gs[0][2] > G and gs[-1][2] > G
        gs = [x[1:3] for x in _groups(fm.make(cs["cut_then_owned"]))]
        assert (st - 5, G) in gs and (st - 5 + G, 9) in gs                    # cut by the second window's start; the owned one behind starts inside the stride
        gs = [x[1:3] for x in _groups(fm.make(cs["cut_hard"]))]
        assert (st - 5, G + 7) in gs
        gs = [x[1:3] for x in _groups(fm.make(cs["hard_over_strides"]))]
        assert (st - G, G + 5) in gs                                          # members st - G .. st - 1 in the first stride range, five in the next
        res = fm.run_model(cs["hard_over_strides"], fm.make(cs["hard_over_strides"]))
        assert res["hard_count"][0] + res["shallow_count"][0] == G + 5
    floors = set((c["floor"], c["dcap"]) for c in _by("seams"))
    assert len(floors) == 9


def test_region_cases():
    for c in _by("regions"):
        inp = fm.make(c)
        counts = [cnt for _, cnt in inp["regions"]]
        st = c["win"] - c["G"]
        assert len(counts) == c["nreg"]
        if c["nreg"] == 16:
            assert counts[0] == 0 and 0 in counts[1:] and counts.count(0) >= 8
        if c["cuts"] == "one_group":
            assert 1 in [len([g for g in _groups(inp) if g[0] == r]) for r in range(16)] and counts[-1] == 0
        if c["cuts"] == "on_stride":
            assert counts[1] == 2 * st and counts[0] == 0
        bases = [b for b, _ in inp["regions"]]
        assert bases == sorted(bases)


def test_dealing_cases_fill_the_regions_they_are_named_for():
    for c in _by("dealing"):
        inp = fm.make(c)
        res = fm.run_model(c, inp)
        assert res["grid"] == c["grid"]
        assert int((res["SA"] != fm.POISON).sum()) == 0 and res["hard_count"][0] == 0          # every group left tied
        used = [r for r in range(16) if res["next_count"][r]]
        assert used == {64: [0], 65: [0, 1], 1024: list(range(16)), 1025: list(range(16))}[c["grid"]]
        if c["grid"] == 1025:
            assert res["next_count"][0] > res["next_count"][1]                             # the wrap to region 0


def test_character_cases():
    for c in _by("chars"):
        inp = fm.make(c)
        res = fm.run_model(c, inp)
        chars = 8 * c["words"] * c["rounds"]
        b, cnt = inp["regions"][0]
        s, d = inp["S"][b:b + cnt].astype(np.int64), inp["C"][b:b + cnt].astype(np.int64) >> 8
        assert set(((s + d) & 7).tolist()) == set(range(8)), c["name"]
        assert bool((s + d + chars > len(inp["T"])).any()) == c["end"], c["name"]
        assert int((res["SA"] != fm.POISON).sum()) >= 2 * c["rounds"] and int(res["next_count"][16]) >= 2 * c["rounds"] + 2, c["name"]
        sizes = sorted(np.bincount(np.unique(res["next"][0][:, 0], return_inverse=True)[1]).tolist())
        assert 2 in sizes and 3 in sizes and 9 in sizes, c["name"]                          # uneven sub-groups; the whole group equal


def test_end_cases_reach_the_end_where_they_say():
    for c in _by("end-w"):
        inp = fm.make(c)
        n = len(inp["T"])
        b, cnt = inp["regions"][0]
        s, d = inp["S"][b:b + cnt].astype(np.int64), inp["C"][b:b + cnt].astype(np.int64) >> 8
        assert c["left"] in (n - (s + d)).tolist(), c["name"]
        last = int(s[(n - (s + d)) == c["left"]].max())
        res = fm.run_model(c, inp)
        head = int(inp["H"][b:b + cnt][s == last][0])
        rows = res["next"][0]
        if c["left"] < 8 * c["words"] * c["rounds"]:                                        # the proper prefix is final, first of its group
            assert int(res["SA"][head]) == last, c["name"]
            assert len(rows[rows[:, 0] == head + 1]) == 2, c["name"]                      # the two members with real zero bytes there stay tied
        else:                                                                             # the pass does not reach the end: all four stay tied
            assert last in rows[rows[:, 0] == head][:, 1].tolist() and len(rows[rows[:, 0] == head]) == 4, c["name"]
    lefts = set(c["left"] for c in _by("end-w2-r4"))
    assert lefts >= set(range(0, 66)) | {-1, -5}
    for c in _by("end-texts"):
        inp = fm.make(c)
        T = inp["T"]
        if c["kind"] == "ab":
            assert bytes(T[:4]) == b"abab" and len(T) == c["n"]
        else:
            assert not T[-300:].any()


def test_depth_cases():
    for c in _by("depths"):
        inp = fm.make(c)
        chars = 8 * c["words"] * c["rounds"]
        gs = _groups(inp)
        depths = set(g[3] for g in gs)
        assert depths >= {0, 1, max(c["floor"] - 1, 0), c["floor"], 48, 255 - chars, 255}, c["name"]
        res = fm.run_model(c, inp)
        new = set((res["next"][0][:, 2] >> 8).tolist())
        assert 255 in new and min(255, chars) in new, c["name"]
        assert res["hard_count"][1] == c["floor"] and gs[-1][3] == c["floor"] and gs[-1][2] > c["G"], c["name"]     # the smallest depth: the list's last entries
        assert [g[3] for g in gs if g[2] > c["G"]].count(c["floor"]) == 1, c["name"]
        assert (res["shallow_count"][0] > 0) == (c["floor"] > 0), c["name"]


def test_emit_cases():
    got_last = noted = missed = 0
    for c in _by("emit"):
        inp = fm.make(c)
        n = len(inp["T"])
        assert sum(cnt for _, cnt in inp["regions"]) == n == c["n"]
        res = fm.run_model(c, inp)
        if c["lf_n"] > 1:
            x = n // c["lf_n"]
            hits = int((res["lf"] != fm.POISON).sum())
            assert res["lf"][0] == fm.POISON and hits <= c["lf_n"] - 1, c["name"]
            noted += hits
            missed += c["lf_n"] - 1 - hits                                               # every suffix n - k x is on the list; those left tied note nothing
            isa = fm.inverse(inp["SA"])
            for k in np.flatnonzero(res["lf"] != fm.POISON):
                assert isa[n - k * x] == res["lf"][k], c["name"]
        else:
            assert (res["lf"] == fm.POISON).all()
        got_last += res["last_char"] != fm.POISON
    assert got_last >= 3 and noted > 300 and missed > 50
    assert set(c["n"] // c["lf_n"] for c in _by("emit") if c["lf_n"] > 1) >= {1, 2, 3, 16, 13, 375, 819}
    assert any(fm.run_model(c, fm.make(c))["pidx"] != fm.POISON for c in _by("emit"))


def test_rank_cases():
    none = finals = second = 0
    for c in _by("rank"):
        inp = fm.make(c)
        n = len(inp["T"])
        res = fm.run_model(c, inp)
        assert (inp["at2"] != 0) == bool(c["at2_on"])
        sizes = [g[2] for g in _groups(inp)]
        assert min(sizes) >= 2 and max(sizes) <= c["G"], c["name"]
        listed = np.concatenate([np.arange(b, b + cnt) for b, cnt in inp["regions"]])
        none += int((res["us"][listed] == fm.NONE).sum())
        finals += int((res["SA"] != fm.POISON).sum())
        if c["text"] == "ab":
            s = inp["S"][listed].astype(np.int64)
            assert n - 1 in (s + inp["at"]).tolist() and n in (s + inp["at"]).tolist(), c["name"]     # a look-up at the last suffix, and one past the end
            assert 0 in inp["rank"][np.minimum(s + inp["at"], n - 1)].tolist(), c["name"]               # rank 0 beside "past the end"
        s = inp["S"][listed].astype(np.int64)
        if c.get("deep"):                                                # a listed member's look-up lands on the largest suffix: rank n - 1
            top = int(inp["SA"][n - 1])
            assert int(inp["rank"][top]) == n - 1 and top - inp["at"] in s.tolist(), c["name"]
            if inp["at2"]:
                assert top - inp["at2"] in s.tolist(), c["name"]
        elif inp["at2"] and c["text"] == "phrase" and "per_region" not in c:                       # members of one old group equal in the first key word and apart in the second
            k1 = np.where(s + inp["at"] < n, inp["rank"][np.minimum(s + inp["at"], n - 1)].astype(np.int64) + 1, 0)
            k2 = np.where(s + inp["at2"] < n, inp["rank"][np.minimum(s + inp["at2"], n - 1)].astype(np.int64) + 1, 0)
            h = inp["H"][listed].astype(np.int64)
            o = np.lexsort((k2, k1, h))
            same = (h[o][1:] == h[o][:-1]) & (k1[o][1:] == k1[o][:-1]) & (k2[o][1:] != k2[o][:-1])
            assert int(same.sum()) >= 5, c["name"]
            second += 1
        if "per_region" in c:
            assert [cnt for _, cnt in inp["regions"]] == [c["per_region"]] * c["nreg"], c["name"]
        # the model's rank[] after the updates is the head slot of every listed suffix's new sub-group
        assert fm.refined_breaks(inp["T"], inp["SA"], res) == 0
    assert none > 100 and finals > 100 and second >= 15


@pytest.mark.parametrize("c", fm.driver_cases(), ids=lambda c: c["name"])
def test_driver_cases_stop_by_the_rule_they_are_named_for(c):
    inp = fm.make_driver(c)
    T, SA = inp["T"], inp["SA"]
    m = len(inp["S"])
    assert fm.list_breaks(T, SA, [(0, m)], inp["S"], inp["P"], inp["H"], inp["C"]) == 0
    res = fm.expect_driver(T, inp["S"], inp["P"], inp["H"], inp["C"], **inp["args"])
    assert (res["passes_done"], res["stop"]) == (c["passes"], c["stop"])
    if c["name"] == "driver-depth-passes":
        assert res["local"] >= 4096                                   # neither "few" nor a rule of proportion: the depth byte's bound ended it
    if c["name"] == "driver-no-pass-holes":
        assert res["park_holes"] == res["shallow"] > 0 and res["route"] == 0
    if c["name"].endswith("local1") or c["name"] in ("driver-wide", "driver-sixteen-regions"):
        assert res["local"] > 0 and res["left"] == 0
    if c["name"].endswith("local0") or c["name"] == "driver-three-quarters":
        assert res["left"] > 0 and res["local"] == 0
    # every entry is accounted for once, finals are placed, what is left is refined
    finals = int((res["SA"] != fm.POISON).sum())
    assert finals + res["parked"] + res["shallow"] - res["park_holes"] + res["local"] == m
    assert fm.placed_breaks(res, SA) == 0
    assert fm.driver_refined_breaks(T, SA, res) == 0


# The mutants of DESIGN.md section 8g, replayed in the model (finmodel.expect_pass(mutant=...)): each must change an output
# that tests/test_gpu_finisher.py compares exactly, in named cases of the buckets listed -- the device is held to the
# unmutated model, so a kernel with the mutant's behaviour fails those buckets' tests.
_MUTANTS = {
    1: ("ownership a <= stride", {"seams-1024-256", "seams-1024-512", "seams-2048-256", "seams-2048-512", "seams-2048-1024", "regions"}, {"next_count"}),
    2: ("group bound off <= G", {"seams-1024-256", "seams-1024-512", "seams-2048-256", "seams-2048-512", "seams-2048-1024", "depths"}, {"hard", "shallow"}),
    3: ("touch order < sfx", {"end-w2-r1", "end-w2-r2", "end-w2-r3", "end-w2-r4", "end-w3-r1", "end-w4-r1", "end-texts"}, {"SA"}),
    4: ("touch bit of the later rounds", {"end-w2-r2", "end-w2-r3", "end-w2-r4", "end-texts"}, {"SA", "next_count"}),
    5: ("depth + one round only", {"chars", "end-w2-r2", "end-w2-r3", "end-w2-r4", "depths"}, {"next[0]"}),
    7: ("lf_note without the correction", {"emit"}, {"lf"}),
    8: ("RANK notes always the suffix", {"rank", "rank-updates"}, {"us", "rank"}),
    9: ("heads count !=", {"chars", "regions", "depths", "emit", "rank"}, {"next_count"}),
}


@pytest.mark.parametrize("mutant", sorted(_MUTANTS))
def test_replayed_mutant_changes_a_compared_output(mutant):
    what, want_buckets, want_outputs = _MUTANTS[mutant]
    hit, outputs = set(), set()
    for c in CASES:
        if c["kind"] == "twins" or c["bucket"] not in want_buckets:
            continue
        inp = fm.make(c)
        ranks = "rank" in inp
        d = fm.differences(fm.run_model(c, inp), fm.run_model(c, inp, mutant=mutant), ranks)
        if d:
            hit.add(c["bucket"])
            outputs |= set(x.split(":")[0] for x in d)
    assert hit == want_buckets, (what, want_buckets - hit)
    assert outputs >= want_outputs, (what, outputs)
