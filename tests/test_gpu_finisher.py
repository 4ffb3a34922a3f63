"""The suffix sorter's finisher on the GPU (-m gpu), launch by launch: k_finish in its chars form (five window / group
shapes, words 2, 3, 4, rounds 1..4) and its RANK form with k_rank_updates, through the hooks bwtc_hip_test_finish_pass /
_local_pass, which share their launch code with finisher_passes / local_pass, and the driver finisher_passes itself
(k_fin_to_hard, k_list_copy) through bwtc_hip_test_finisher, held to tests/finmodel.py by exact
comparison: finals (SA, out, pidx, last_char, lf), every count, both smallest depths and the heads count exactly; the hard
and the shallow list as sets of (S, H, P, C); the next list per region as the set of its groups, after the invariant the
next pass relies on.  What the device may choose freely (the order of workgroups in a region, which tied member gets
which P) is not pinned.  On top of that the device's own output is held to *placed* and *refined*, which come from the
true suffix array alone.  The named cases and their inputs are finmodel.cases() / make(); tests/test_finmodel.py holds
the model to sorted() and every family of cases to the edge it is named for.  The hooks check k_finish's contracts on the
host and guard every array the kernel may write with canaries (a changed one raises)."""
import numpy as np
import pytest

import finmodel as fm
from bwtc_amd import hip

pytestmark = pytest.mark.gpu


def _run(ctx, c):
    inp = fm.make(c)
    want = fm.run_model(c, inp)
    extra = {k: inp[k] for k in ("rank", "at", "at2") if k in inp}
    got = ctx.test_finish_pass(inp["T"], inp["regions"], inp["S"], inp["P"], inp["H"], inp["C"], **inp["args"], **extra)
    ranks = "rank" in inp
    have = fm.canon(got, len(inp["T"]), ranks)
    bad = fm.differences(want, have, ranks)
    assert not bad, "%s: differs from the model in %s" % (c["name"], bad)
    assert fm.placed_breaks(have, inp["SA"]) == 0, c["name"]
    assert fm.refined_breaks(inp["T"], inp["SA"], have) == 0, c["name"]
    return inp, want, have


def _bucket(ctx, bucket):
    cs = [c for c in fm.cases() if c["bucket"] == bucket]
    assert cs
    for c in cs:
        _run(ctx, c)


@pytest.mark.parametrize("bucket", fm.buckets("seams"))
def test_window_seams(hip_ctx, bucket):
    """Per shape: lists of 1, 2, stride - 1, stride, stride + 1, win - 1, win, win + 1, 2 stride - 1 and 2 stride + 1
    entries; groups of 1, 2, G - 1, G, G + 1, 2 G, win + 1 and 3 stride + 5 members in both orders; groups of 2, G and
    G + 1 members starting at positions 0, 1, stride - 1, stride, stride + 1, 2 stride - 1, 2 stride, 2 stride + 1 (window
    positions 0, 1, stride - 1 of the first three windows and the last owned position); an owned and a hard group first
    and last in the list; a group of G and one of 2 cut by the second window's start with an owned group directly behind;
    a hard group cut by the window's start; a hard group whose first G members lie in one stride range and the rest in
    the next, and one over three stride ranges (each member appended exactly once).  Words, rounds, floor 0 / 12 / 48 and
    claimed depths 0 / up to 40 / up to 60 rotate over the cases."""
    _bucket(hip_ctx, bucket)


def test_input_regions(hip_ctx):
    """Per shape: the list in 2, 3 and 16 regions with gaps between them, empty regions first, between and last; a
    region of one group; a region that ends on a multiple of the stride."""
    _bucket(hip_ctx, "regions")


@pytest.mark.parametrize("c", [c for c in fm.cases() if c["bucket"].startswith("dealing")], ids=lambda c: c["name"])
def test_output_dealing(hip_ctx, c):
    """Every group left tied (pairs that share 52 to 128 characters), grids of 64, 65, 1024 and 1025 workgroups in the
    narrow and in the wide shape: the second region, all sixteen, the wrap to region 0 -- 786 816 entries over 1.33 MB of
    text narrow, 1 049 088 over 1.77 MB wide.  (The device's part is milliseconds; the first large case of a shape also
    makes its text's suffix array in numpy and takes 1.3 s narrow, 1.8 s wide on the GPU machine, the others under a second.)"""
    _run(hip_ctx, c)


def test_characters(hip_ctx):
    """Per (words, rounds): groups of seven whose members differ only in the first byte or only in the last byte of a
    round (and in bytes 7 and 8), by 0x00 < 0x7F < 0x80 < 0xFF with two and three members equal; a group wholly equal;
    one wholly distinct; sub-groups that split again in every later round; every alignment (s + depth) & 7; once with
    no member of the window near the end of T (the lean loop) and once with one (the other loop)."""
    _bucket(hip_ctx, "chars")


@pytest.mark.parametrize("bucket", fm.buckets("end"))
def test_end_of_text(hip_ctx, bucket):
    """Per (words, rounds): a group whose last member ends n - (s + depth) = 0 .. chars + 1 characters after its depth
    (s + depth = n, n - 1, ...: past the end in round 1, 2, 3, 4 only, or not at all) and 1 and 5 characters before it
    (s + depth above n), beside two members that have real zero bytes where it has run out of text and one that is
    greater.  end-texts: abab...ab of 500, 501 and 2300 bytes and one with a tail of zeros, every suffix listed; a text
    that ends in 300 zero bytes."""
    _bucket(hip_ctx, bucket)


def test_depths_and_floors(hip_ctx):
    """Per (words, rounds) and floor 0, 12, 48: owned groups of depth 0, 1, floor - 1, floor, 48, 254 - chars, 255 - chars,
    256 - chars (saturation) and 255; hard groups of depth floor - 1 (shallow), floor + 1, 48 or more and, as the list's
    last entries, floor: the smallest depth comes from the last wave of the last workgroup."""
    _bucket(hip_ctx, "depths")


def test_emission(hip_ctx):
    """Every suffix of the text on the list, so that suffix 0, slot n - 1 (out_n = n - 1: last_char) and every suffix
    n - k x are there, final or not: lf_n 0, 1, 2, 3, 5, 8, 256 with x = 1, 2, 3, 13, 16, 375 and 819 (n / lf_n with and
    without a remainder), out_n = n and n - 1."""
    _bucket(hip_ctx, "emit")


@pytest.mark.parametrize("bucket", fm.buckets("rank"))
def test_rank_passes(hip_ctx, bucket):
    """k_finish<RANK> and k_rank_updates, per shape: groups of 2 .. G members, at 1, 4, 16, at2 zero and 2 at, 1, 2 and 16
    regions with empty ones; abab...ab with look-ups at n - 1 and past the end and rank 0 beside "past the end"; members
    with nothing below them (kFinNone); rank-updates: regions of 2, 1023, 1024 and 1025 entries, 2 and 16 of them.  us,
    ur and rank[] after the updates compared exactly."""
    _bucket(hip_ctx, bucket)


def _refused(call):
    with pytest.raises(hip.BwtcHipError) as e:
        call()
    return e.value.code


def test_contract_refusals(hip_ctx):
    """A list that breaks what k_finish assumes is refused before anything is launched (-1), and the context still
    works afterwards."""
    ctx = hip_ctx
    c = [c for c in fm.cases() if c["name"] == "seam-1024-256-sizes"][0]
    inp = fm.make(c)
    T, regions, a = inp["T"], inp["regions"], inp["args"]
    S, P, H, C = inp["S"], inp["P"], inp["H"], inp["C"]
    b = regions[0][0]
    run = lambda T=T, regions=regions, S=S, P=P, H=H, C=C, **kw: ctx.test_finish_pass(T, regions, S, P, H, C, **dict(a, **kw))

    def changed(arr, i, v):
        arr = arr.copy()
        arr[i] = v
        return arr
    assert _refused(lambda: run(window=1024, group=1024)) == -1
    assert _refused(lambda: run(window=2048, group=128)) == -1
    assert _refused(lambda: run(words=5)) == -1
    assert _refused(lambda: run(words=3, rounds=2)) == -1
    assert _refused(lambda: run(words=2, rounds=5)) == -1
    assert _refused(lambda: run(out_n=len(T) - 2)) == -1
    assert _refused(lambda: run(lf_n=257)) == -1
    assert _refused(lambda: run(regions=[(b, 0)])) == -1                                          # no entries
    assert _refused(lambda: run(regions=[(b, 100), (b + 50, 100)])) == -1                         # regions overlap
    assert _refused(lambda: run(regions=[(b + 500, 100), (b, 100)])) == -1                        # descend
    assert _refused(lambda: run(S=changed(S, b + 3, len(T)))) == -1                               # S >= n
    assert _refused(lambda: run(S=changed(S, b + 3, S[b + 4]))) == -1                             # S twice
    assert _refused(lambda: run(P=changed(P, b + 3, len(T)))) == -1
    k = int(np.flatnonzero(P[b:] != H[b:])[0]) + b                                                # a second member of a group
    assert _refused(lambda: run(P=changed(P, k, P[k] + 1))) == -1                                 # P != H + j
    assert _refused(lambda: run(C=changed(C, k, C[k] ^ 0x100))) == -1                             # two depths in a group
    assert _refused(lambda: run(H=changed(H, k, H[k] + 1))) == -1                                 # a run that does not start at its head
    big = np.zeros((64 << 20) + 1024, np.uint8)
    assert _refused(lambda: run(T=big)) == -1                                                     # no room for the canaries
    r = [c for c in fm.cases() if c["name"] == "rank-1024-256-at4-two1"][0]
    ri = fm.make(r)
    rr = lambda **kw: ctx.test_finish_pass(ri["T"], ri["regions"], ri["S"], ri["P"], ri["H"], ri["C"],
                                           **dict(dict(ri["args"], rank=ri["rank"], at=ri["at"], at2=ri["at2"]), **kw))
    assert _refused(lambda: rr(at=0)) == -1
    assert _refused(lambda: rr(at2=ri["at"])) == -1
    assert _refused(lambda: rr(at=0x7FFFFFF0, at2=0xFFFFFFE0)) == -1
    assert _refused(lambda: rr(rank=changed(ri["rank"], 5, len(ri["T"])))) == -1
    assert _refused(lambda: rr(group=512, window=2048, words=3)) == -1
    one = fm.make([c for c in fm.cases() if c["name"] == "seam-1024-256-sizes"][0])              # singletons and groups above the bound
    assert _refused(lambda: ctx.test_finish_pass(one["T"], one["regions"], one["S"], one["P"], one["H"], one["C"], window=1024, group=256,
                                                 rank=np.zeros(len(one["T"]), np.uint32), at=1)) == -1
    # and the context still works
    _run(ctx, c)
    _run(ctx, r)


@pytest.mark.parametrize("c", fm.driver_cases(), ids=lambda c: c["name"])
def test_driver(hip_ctx, c):
    """finisher_passes through bwtc_hip_test_finisher against the model's own pass iterated under the restated stop
    rules: lists that stop by "fewer than 4096 left" (all five shapes, kept as the local list and parked), by the
    three-fifths rule after the second pass, the three-quarters rule after the third, the depth byte's bound (three passes
    of 64 characters), max_passes 1 and 0 (a list no pass has looked at: shallow entries leave holes, park_holes); a
    second pass over a list the first left in 16 regions (786 816 entries) that then becomes the local list through
    k_list_copy; the wide shape.  FinOutcome, passes_done, stats.route, every count and smallest depth and the
    emissions exactly; the parked, shallow and local lists as sets."""
    inp = fm.make_driver(c)
    want = fm.expect_driver(inp["T"], inp["S"], inp["P"], inp["H"], inp["C"], **inp["args"])
    got = hip_ctx.test_finisher(inp["T"], inp["S"], inp["P"], inp["H"], inp["C"], **inp["args"])
    have = fm.canon_driver(got)
    bad = fm.driver_differences(want, have)
    assert not bad, "%s: differs from the model in %s" % (c["name"], bad)
    assert fm.placed_breaks(got, inp["SA"]) == 0
    assert fm.driver_refined_breaks(inp["T"], inp["SA"], have) == 0
