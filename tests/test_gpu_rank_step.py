"""The suffix sorter's ranking step and round kernels on the GPU (-m gpu), kernel by kernel: k_rerank_reduce,
k_rerank_scan_tiles<0>, <1> and k_rerank_apply through bwtc_hip_test_rank_pass (launch_rerank, rank_step's own launch
code), the scan alone through _rank_scan, k_gather_key2 / k_gather_text / k_gather_dense through _round_keys,
k_scatter_pairs / k_scatter_dense through _rank_scatter and rank_step<u64, false> itself once per route through _round, held to tests/rankmodel.py by exact comparison: the aggregates as
apply reads them, both counts, rank[] / pairs / records, the next list, SA, out, pidx, last_char and lf[], poison where
the form writes nothing.  k_gather_dense's order inside a chunk of 2048 is free and compared as a multiset per chunk; the
scatters are compared through rank[].  The device's own output is also held to *placed* and *refined*, which come from the
true suffix array alone.  tests/test_rankmodel.py holds the model to sorted() and a slot-by-slot restatement, and every
named case to its edge.  The hooks check the kernels' contracts on the host and guard every array a kernel may write
with canaries (a changed one raises)."""
import numpy as np
import pytest

import rankmodel as rm
from bwtc_amd import hip

pytestmark = pytest.mark.gpu

CASES = rm.pass_cases()


def _device_pass(ctx, T, L, mode, emit, out_n=None, lf_n=0, rec_shift=0, plane=True):
    return ctx.test_rank_pass(T, L["keys"], rm.device_idx(L), init=L["init"], split=L["split"], mode=mode, emit=emit, w=L["w"], aglob=L["aglob"],
                              short_len=L["short_len"], kmask=L["kmask"], long=L["long"], inv_lut=L["inv_lut"] if emit == 3 else None,
                              out_n=out_n, lf_n=lf_n, rec_shift=rec_shift, plane=plane)


def _check_pass(ctx, T, L, mode, emit, depth, tag, **kw):
    got = _device_pass(ctx, T, L, mode, emit, **kw)
    want = rm.expect_pass(T, L, mode, emit, **kw)
    bad = rm.differences(want, got, mode)
    assert not bad, "%s: differs from the model in %s" % (tag, bad)
    SA = rm.sa_of(T)
    assert rm.placed_breaks(T, SA, got, emit, kw.get("out_n")) == 0, tag
    assert rm.refined_breaks(T, SA, *rm.left_of(got, mode), want["_depth"] if isinstance(depth, str) else depth) == 0, tag
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_ranking_pass_sizes_groups_and_seams(hip_ctx, name):
    """The named cases of rankmodel.pass_cases(): list sizes 1 .. 17 x 2048 + 5, groups of 2 .. 2 x 2048 + 3 members, a group
    starting at the lane, iteration, wave-chunk and tile seams - 1 / 0 / + 1, a group over three whole tiles with a
    singleton behind it, a head in a tile's last slot, all singletons, one group, a tile with nothing active and one with
    nothing finished, the short-suffix rule at short_len 1, 4 and 8, payload above kmask -- each as MODE 0 (rank[] from the
    kernel) and MODE 3 (the raw list) with T[s - 1] emitted and slot n - 1 going to last_char."""
    c = CASES[name]
    L = rm.make_list(c)
    for mode in (0, 3):
        _check_pass(hip_ctx, c["T"], L, mode, 2, L["claim"], "%s mode %d" % (name, mode), out_n=L["n"] - 1)


@pytest.mark.parametrize("form", ["u32", "u64", "u64_payload", "split", "gram", "gram_split", "levels", "levels_split", "code", "code_split"])
def test_ranking_pass_every_initial_form_mode_and_emit(hip_ctx, form):
    """n = 65536 + 1025 (odd; the suffix numbers' upper bits in play), every MODE with both emit forms rank_step pairs with
    the list's form: u32 and u64 keys (0, 2), 16-bit halves with the upper bits at bit 48 (0, 2), long items of the gram form
    and with per-item levels 0..7, whole and split (0, 3; wmask of 9 bits under random upper bits; an inv_lut that is no
    identity); long items of the code form from codemodel.py's keys, second words and levels over a structured text of
    30 001 bytes, whole and split, held to the depth their levels claim.  The split forms also run at an even size."""
    texts = [rm.code_forms()[0]] if "code" in form else [rm.form_text()] + ([rm.form_text(6000, 8)] if "split" in form else [])
    for T in texts:
        L, e = rm.code_forms()[1][form] if "code" in form else rm.init_forms(T)[form]
        for mode in range(4):
            for emit in (0, e):
                kw = dict(out_n=L["n"] - (mode & 1), lf_n=(0, 5, 256, 2)[mode], rec_shift=3 * mode, plane=mode != 2 or emit != 0)
                got = _check_pass(hip_ctx, T, L, mode, emit, L["claim"], "%s n %d mode %d emit %d" % (form, L["n"], mode, emit), **kw)
                if mode == 3 and L["long"] is not None:                # the depth byte rides above the character
                    q = int(got["counts"][0])
                    assert q > 0 and set((got["achr"][:q] >> 8).tolist()) == set((L["depth"] & 0xFF)[rm.structure(L)[3]].tolist())


@pytest.mark.parametrize("carry", [False, True])
def test_ranking_pass_rounds(hip_ctx, carry):
    """A round's list (the model's own initial ranking, sorted by (group, rank[s + k] + 1)): aglob with gaps, heads read
    through aglob across tile seams, every MODE with emit 0, 2 and -- where the keys carry the character -- 1."""
    T = rm.form_text(30000, 8)
    L, rank, h = rm.round_list(T, 4, carry)
    assert L["m"] > 3 * rm.TILE
    for mode in range(4):
        for emit in ((0, 2, 1) if carry else (0, 2)):
            _check_pass(hip_ctx, T, L, mode, emit, 2 * h, "round carry %d mode %d emit %d" % (carry, mode, emit), lf_n=3, rec_shift=5)


def test_ranking_pass_emissions(hip_ctx):
    """Suffix 0 finished in slot n - 1 = out_n (pidx and last_char) and still active (pidx stays poison); lf_n 0, 1, 2, 3,
    5, 256 with x = n / lf_n of 1, 3, 13, 819; emit 1 with all 256 byte values in bits 56..63."""
    for name, T in rm.emit_texts().items():
        L = rm.list_sigma(T, rm.sa_of(T), rm.K)
        _check_pass(hip_ctx, T, L, 0, 2, rm.K, name, out_n=len(T) - 1)
        _check_pass(hip_ctx, T, L, 1, 2, rm.K, name, out_n=len(T))
    for n, lf_n in rm.LF_CASES:
        T = rm.random_text(n, 4, n + lf_n, tail=2)
        _check_pass(hip_ctx, T, rm.list_sigma(T, rm.sa_of(T), 8), 0, 2, 8, "lf %d %d" % (n, lf_n), lf_n=lf_n)
    T = rm.bytes_text(20000, 3)
    L, rank, h = rm.round_list(T, 1, True)
    _check_pass(hip_ctx, T, L, 0, 1, 2, "bytes", out_n=len(T) - 1, lf_n=256)


def test_ranking_pass_contracts(hip_ctx):
    """Lists the hook refuses before anything is launched."""
    T = rm.form_text(6000, 8)
    L = rm.list_sigma(T, rm.sa_of(T), 4)
    R, rank, h = rm.round_list(T, 4, True)

    def refused(L, mode=0, emit=0, **kw):
        with pytest.raises(hip.BwtcHipError) as e:
            _device_pass(hip_ctx, T, L, mode, emit, **kw)
        return e.value.code == -1
    twice = dict(L, sfx=np.concatenate((L["sfx"][:1], L["sfx"][:-1])))
    assert refused(twice)
    assert refused(dict(L, sfx=L["sfx"] + 1))                               # a suffix number of n
    assert refused(dict(L, m=L["m"] - 1, keys=L["keys"][:-1], sfx=L["sfx"][:-1]))    # INIT with m < n
    assert refused(L, emit=1) and refused(L, emit=3)                        # forms rank_step never pairs
    assert refused(L, emit=2, out_n=L["n"] - 2) and refused(L, emit=2, lf_n=257) and refused(L, mode=2, rec_shift=32)
    assert refused(dict(R, aglob=R["aglob"][::-1].copy())) and refused(dict(R, aglob=np.minimum(R["aglob"] + L["n"], 2 ** 32 - 1)))
    assert refused(dict(R, split=True)) and refused(R, emit=3)


SCAN_KINDS = ("zeros", "random", "sum_max", "max_first", "max_part_end")


@pytest.mark.parametrize("nt", rm.SCAN_TILES)
def test_scan_of_the_aggregates(hip_ctx, nt):
    """k_rerank_scan_tiles<0> and <1> over 1 .. 8193 aggregates (the hand-over between workgroups at 4096): zeros, what a
    reduce leaves, sums reaching 2^32 - 1, a max only in the first entry, a max only in the last entry of a part."""
    for kind in SCAN_KINDS:
        a, b, c = rm.scan_inputs(nt, kind)
        ea, eb, ec, parts, counts = rm.expect_scan(a, b, c)
        ga, gb, gc, gparts, gcounts = hip_ctx.test_rank_scan(a, b, c)
        tag = "%d %s" % (nt, kind)
        assert np.array_equal(ga, ea) and np.array_equal(gb, eb), tag
        assert np.array_equal(gc, ec), tag
        assert np.array_equal(gparts[:len(parts)], parts) and (gparts[len(parts):] == rm.P32).all(), tag
        assert np.array_equal(gcounts, counts), tag
    with pytest.raises(hip.BwtcHipError):
        hip_ctx.test_rank_scan(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32))


def test_scan_up_to_what_the_context_reserved():
    """A context for blocks of 8192 x 2048 - 1 bytes reserves 8193 aggregates: the scan of exactly that many (the canaries
    lie in the arrays' spare words), and one more is refused."""
    with hip.Context(device=0, max_block_size=8192 * 2048 - 1) as ctx:
        a, b, c = rm.scan_inputs(8193, "random")
        ea, eb, ec, parts, counts = rm.expect_scan(a, b, c)
        ga, gb, gc, gparts, gcounts = ctx.test_rank_scan(a, b, c, parts_cap=9)
        assert np.array_equal(ga, ea) and np.array_equal(gb, eb) and np.array_equal(gc, ec)
        assert np.array_equal(gparts, parts) and np.array_equal(gcounts, counts)
        with pytest.raises(hip.BwtcHipError) as e:
            ctx.test_rank_scan(np.zeros(8194, np.uint32), np.zeros(8194, np.uint32), np.zeros(8194, np.uint32), parts_cap=9)
        assert e.value.code == -1


def _key_list(n, m, h, seed):
    """m distinct suffixes (those whose s + h lies at n - 1, n and past it among them), ascending groups, a permutation as
    rank[] with rank 0 beside the suffix that looks past the end."""
    rng = np.random.default_rng(seed)
    hh = min(h, n)
    must = [s for s in (n - 1 - hh, n - hh, n - hh + 1, n - 1, 0) if 0 <= s < n]
    rest = np.setdiff1d(rng.permutation(n)[:m + 8], must)[:max(0, m - len(set(must)))]
    aidx = rng.permutation(np.concatenate((np.unique(must), rest)).astype(np.uint32))[:m]
    agrp = np.sort(rng.integers(0, max(1, m // 3), m)).astype(np.uint32)
    rank = rng.permutation(n).astype(np.uint32)
    if 0 <= n - 1 - hh:
        rank[n - 1] = 0
    return aidx, agrp, rank


@pytest.mark.parametrize("m", [1, 1023, 1024, 1025, 4097])
def test_round_keys_key2(hip_ctx, m):
    """k_gather_key2: s + h at n - 1, at n and past it, h = 0xFFFFFFFF, rank 0 beside "past the end", the carried character
    on and off, b2 = rank_bits(n) and one more."""
    n = 5000
    T = rm.random_text(n, 4, 6)
    for h in (1, 4, 4999, 5000, 0xFFFFFFFF):
        aidx, agrp, rank = _key_list(n, m, h, m + (h & 255))
        achr = (np.arange(m) * 37 & 255).astype(np.uint8)
        for b2 in (rm.rank_bits(n), rm.rank_bits(n) + 1):
            for ch in (None, achr):
                got = hip_ctx.test_round_keys(T, 0, h, b2, aidx=aidx, agrp=agrp, rank=rank, achr=ch)
                assert np.array_equal(got, rm.expect_key2(T, aidx, agrp, rank, ch, h, b2)), (m, h, b2, ch is not None)
    with pytest.raises(hip.BwtcHipError):
        hip_ctx.test_round_keys(T, 0, 4, rm.rank_bits(n) - 1, aidx=aidx, agrp=agrp, rank=rank)
    with pytest.raises(hip.BwtcHipError):
        hip_ctx.test_round_keys(T, 0, 4, rm.rank_bits(n), aidx=aidx + np.uint32(n), agrp=agrp, rank=rank)


_stretch_lengths = rm.stretch_lengths


@pytest.mark.parametrize("p", [1, 2, 7])
def test_round_keys_run_step(hip_ctx, p):
    """RunKeys mode 1 (the step's closed-form keys, with and without rank[]) and mode 2 (the look-up behind the stretch) in
    k_gather_key2, period 1, 2 and 7: k = h - 1, h, h + 1, a stretch ending at n, falling and rising behind the stretch; mode
    2 with k below, at and above h_split and h below and above k."""
    rng = np.random.default_rng(40 + p)
    unit = rng.integers(1, 4, p, dtype=np.uint8)
    parts = []
    for i in range(260):                                           # stretches of 1 .. 14 periods' characters, a breaker of 0 or 5 between
        parts += [np.resize(unit, int(rng.integers(1, 15)) + p), np.array([0 if i % 2 else 5], np.uint8)]
    T = np.concatenate(parts + [np.resize(unit, 9 + p)])           # the last stretch ends at n
    n = len(T)
    k = _stretch_lengths(T, p)
    h = 8
    assert {h - 1, h, h + 1} <= set(k.tolist()) and int(k[n - 9 - p]) == 9 + p
    ends = np.arange(n) + k
    longs = k >= h
    rising = longs & (ends < n) & (T[np.minimum(ends, n - 1)] > T[np.minimum(ends, n - 1) - p])
    assert rising.any() and (longs & ~rising & (ends < n)).any() and (longs & (ends >= n)).any()
    aidx, agrp, rank = _key_list(n, 3000, h, 3)
    b2 = rm.rank_bits(n) + 1
    for rk in (rank, None):
        got = hip_ctx.test_round_keys(T, 0, h, b2, aidx=aidx, agrp=agrp, rank=rk, run_mode=1, k=k, p=p)
        assert np.array_equal(got, rm.expect_key2(T, aidx, agrp, rk, None, h, b2, 1, k, 0, p)), (p, rk is not None)
    for h2, hs in ((8, 8), (16, 8), (4, 4), (32, 6)):
        assert (k < hs).any() and (k == hs).any() and (k > hs).any() and (k[aidx] < h2).any() and ((k[aidx] > h2).any() or h2 > 8)
        got = hip_ctx.test_round_keys(T, 0, h2, b2 - 1, aidx=aidx, agrp=agrp, rank=rank, achr=(aidx & 255).astype(np.uint8), run_mode=2, k=k, h_split=hs, p=p)
        assert np.array_equal(got, rm.expect_key2(T, aidx, agrp, rank, (aidx & 255).astype(np.uint8), h2, b2 - 1, 2, k, hs, p)), (p, h2, hs)
    with pytest.raises(hip.BwtcHipError):                           # k[s] > n - s
        hip_ctx.test_round_keys(T, 0, h, b2, aidx=aidx, agrp=agrp, rank=rank, run_mode=1, k=k + np.uint32(1), p=p)


@pytest.mark.parametrize("c", [1, 2, 3, 4, 5, 6])
def test_round_keys_text(hip_ctx, c):
    """k_gather_text with c = 1..6 characters: 0 .. c of them past the end, every alignment of s + h, with and without the
    carried character, and the h_split form behind a run."""
    n = 4099
    T = rm.random_text(n, 250, 12)
    T[100:160] = 9
    k = _stretch_lengths(T, 1)
    for h in (0, 3, 13):
        near = np.arange(n - h - 8, n)                              # s + h from n - 8 on, past n where h > 0
        aidx = np.concatenate((near, np.arange(96, 170), np.arange(1000, 1000 + 700))).astype(np.uint32)
        agrp = (np.arange(len(aidx)) // 100).astype(np.uint32)      # (six characters and a carried one leave a group four bits)
        over = np.minimum(c, np.maximum(0, aidx.astype(np.int64) + h + c - n))
        assert set(over.tolist()) == set(range(c + 1 if h else c)) and set(((aidx + h) & 7).tolist()) == set(range(8))
        for ch in (None, (aidx * 3 & 255).astype(np.uint8)):
            got = hip_ctx.test_round_keys(T, 1, h, c, aidx=aidx, agrp=agrp, achr=ch)
            assert np.array_equal(got, rm.expect_text(T, aidx, agrp, ch, h, c)), (c, h)
        if h >= 3:
            got = hip_ctx.test_round_keys(T, 1, h, c, aidx=aidx, agrp=agrp, run_mode=2, k=k, h_split=3)
            assert np.array_equal(got, rm.expect_text(T, aidx, agrp, None, h, c, 2, k, 3)), (c, h)
    with pytest.raises(hip.BwtcHipError):
        hip_ctx.test_round_keys(T, 1, 2, 7, aidx=aidx, agrp=agrp)


@pytest.mark.parametrize("chunks", [1, 7, 8, 9, 17])
def test_round_keys_dense(hip_ctx, chunks):
    """k_gather_dense over 1 .. 17 chunks of 2048 records (the XCD dealing leaves workgroups without a chunk): finished
    records among them, T[s - 1] emitted with s = 0 in the list, bin_shift 0, 4 and 8; per chunk the multiset of (key, value)."""
    n = 17 * 2048 + 100
    T = rm.random_text(n, 200, 5)
    rng = np.random.default_rng(chunks)
    m = (chunks - 1) * 2048 + (1, 2047, 2048, 5, 300)[chunks % 5]
    s = np.sort(rng.permutation(np.arange(1, n))[:m - 1])
    s = np.concatenate(([0], s))
    for lo in range(0, m, 1024):
        s[lo:lo + 1024] = rng.permutation(s[lo:lo + 1024])
    rec = (s.astype(np.uint64) << np.uint64(32)) | rng.integers(0, n, m, dtype=np.uint64)
    val = np.where(rng.random(m) < 0.3, 0xFFFFFFFF, np.sort(rng.integers(0, m // 2 + 1, m))).astype(np.uint32)
    val[np.flatnonzero(s == 0)] = 0                                  # the record of suffix 0 is active: T[s - 1] is not read for it
    assert int((s == 0).sum()) == 1 and val[np.flatnonzero(s == 0)[0]] == 0
    rank = rng.permutation(n).astype(np.uint32)
    b2 = rm.rank_bits(n)
    for h, emit, bs in ((1, True, 0), (64, False, 4), (n - 5, True, 8), (0xFFFFFFFF, True, 4)):
        gk, gv = hip_ctx.test_round_keys(T, 2, h, b2, rec=rec, val=val, rank=rank, emit=emit, bin_shift=bs)
        wk, wv = rm.expect_dense(T, rec, val, rank, h, b2, emit)
        a, b = rm.chunk_multisets(gk, gv), rm.chunk_multisets(wk, wv)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (chunks, h, emit, bs)


@pytest.mark.parametrize("chunks", [1, 7, 8, 9, 15, 16, 17])
def test_window_scatters(hip_ctx, chunks):
    """k_scatter_pairs and k_scatter_dense over 1 .. 17 chunks (the XCD dealing's empty workgroups), bin_shift 0, 4 and 8, a
    last chunk of one item and of 2048, all destinations in one bin; compared through rank[], untouched elsewhere."""
    n = 40000
    preset = np.random.default_rng(9).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    for last in (1, 2048, 777):
        for bs, one_bin in ((0, False), (4, False), (8, False), (8, True)):
            if one_bin and chunks > 1:
                continue
            where, what = rm.scatter_case(chunks, min(last, 256) if one_bin else last, n, bs, one_bin)
            want = preset.copy()
            want[where] = what
            assert np.array_equal(hip_ctx.test_rank_scatter(preset, where=where, what=what, bin_shift=bs), want), ("pairs", chunks, last, bs)
            rec = (where.astype(np.uint64) << np.uint64(32)) | what.astype(np.uint64)
            assert np.array_equal(hip_ctx.test_rank_scatter(preset, rec=rec, bin_shift=bs), want), ("dense", chunks, last, bs)
    with pytest.raises(hip.BwtcHipError):
        hip_ctx.test_rank_scatter(preset, where=np.array([5, 5], np.uint32), what=np.array([1, 2], np.uint32))
    with pytest.raises(hip.BwtcHipError):
        hip_ctx.test_rank_scatter(preset, where=np.array([n], np.uint32), what=np.array([1], np.uint32))


@pytest.mark.parametrize("kind", ["phrases", "runs", "bytes"])
def test_chain_of_device_steps_ends_at_the_true_suffix_array(hip_ctx, kind):
    """The model's own texts through the initial ranking and every doubling round until nothing is active, every step on the
    device and fed to the next (the keys between them from k_gather_key2 on the device, sorted on the host): the final SA,
    the transform's bytes, pidx, last_char and the LF powers are the true ones."""
    T = dict(phrases=rm.form_text(9000, 5), runs=rm.runs_text([40, 9, 2100, 5], tail=7), bytes=rm.bytes_text(6000, 2))[kind]
    n = len(T)
    SA = rm.sa_of(T)
    L0 = rm.list_sigma(T, SA, 1 if kind == "bytes" else 4)

    def step(L, emit):
        got = _device_pass(hip_ctx, T, L, 0, emit, out_n=n - 1, lf_n=5)
        want = rm.expect_pass(T, L, 0, emit, out_n=n - 1, lf_n=5)
        assert not rm.differences(want, got, 0)
        return got

    def keys(aidx, agrp, rank, achr, h, b2):
        return hip_ctx.test_round_keys(T, 0, h, b2, aidx=aidx, agrp=agrp, rank=rank, achr=achr)
    got_SA, out, pidx, last_char, lf, rounds = rm.chain(T, L0, step=step, out_n=n - 1, lf_n=5, key2=keys)
    assert rounds >= 2 and np.array_equal(got_SA, SA)
    want = np.where(SA > 0, T[np.maximum(SA.astype(np.int64) - 1, 0)], 0)
    assert np.array_equal(out[:n - 1], want[:n - 1]) and last_char == int(want[n - 1]) and pidx == int(np.flatnonzero(SA == 0)[0])
    isa = np.argsort(SA)
    assert all(lf[q] == isa[n - q * (n // 5)] for q in range(1, 5))


def test_window_scatters_one_bin_full_chunk(hip_ctx):
    """2048 and 2049 destinations that all fall into ONE of win_places' 256 bins (the most its LDS counter and its base scan
    take), bin_shift 0 and 4 (at 8 a bin's 2049 destinations would need a block of 128 MiB)."""
    for bs in (0, 4):
        n = (2060 << (8 + bs)) + 77
        rng = np.random.default_rng(bs)
        preset = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        for m in (2048, 2049):
            low = int(rng.integers(0, 1 << bs)) if bs else 0
            where = ((rng.permutation(2060)[:m].astype(np.int64) << (8 + bs)) | (5 << bs) | low).astype(np.uint32)
            assert len(set(((where >> bs) & 255).tolist())) == 1
            what = rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32)
            want = preset.copy()
            want[where] = what
            assert np.array_equal(hip_ctx.test_rank_scatter(preset, where=where, what=what, bin_shift=bs), want), ("pairs", bs, m)
            rec = (where.astype(np.uint64) << np.uint64(32)) | what.astype(np.uint64)
            assert np.array_equal(hip_ctx.test_rank_scatter(preset, rec=rec, bin_shift=bs), want), ("dense", bs, m)


DRIVER = rm.driver_cases()


@pytest.mark.parametrize("window_bits", [4, 16])
@pytest.mark.parametrize("name", sorted(DRIVER))
def test_driver_routes(hip_ctx, name, window_bits):
    """rank_step<u64, false> once per route, pairs_min lowered to the list's size (or one above it), window_bits 4 and 16:
    short; pairs with the partition sort and (n = 4096, so two tiles) without; dense with and without the carried
    character; text; text with the run step; a doubling round behind a run step; raw.  RankResult, the next list as sorted
    (where the dense route leaves the order among equal keys free: as pairs), the raw list, rank[] exact for every suffix
    of the list and untouched elsewhere, the emissions; the device's output held to placed and refined."""
    c = DRIVER[name]
    T, L, rank, kw = rm.make_driver(c)
    pm = c["pm"](L["m"])
    want = rm.expect_round(T, L, rank, pairs_min=pm, **kw)
    assert want["route"] == c["route"] and L["m"] >= 3 * rm.TILE or name == "pairs_unsorted"
    have = hip_ctx.test_round(T, L["keys"], L["sfx"], L["aglob"], rank, pairs_min=pm, window_bits=window_bits, **kw)
    bad = rm.round_differences(want, have)
    assert not bad, "%s: differs from the model in %s" % (name, bad)
    SA = rm.sa_of(T)
    assert rm.placed_breaks(T, SA, have, 1 if kw["emit"] else 0, kw["out_n"]) == 0
    assert rm.refined_breaks(T, SA, *rm.round_left(have, want["route"] == "raw"), None) == 0
    touched = np.zeros(len(T), bool)
    touched[L["sfx"]] = want["route"] != "raw"
    assert np.array_equal(have["rank"][~touched], np.asarray(rank)[~touched])


def test_driver_restores_its_knobs_and_refuses(hip_ctx):
    """A transform after a driver call with pairs_min 1 and window_bits 4 gives the bytes it gave before (the knobs are put
    back); lists and knobs the hook refuses."""
    data = rm.form_text(50000, 3)
    before = hip_ctx.bwt_block(data, 8)
    T, L, rank, kw = rm.make_driver(DRIVER["dense"])
    hip_ctx.test_round(T, L["keys"], L["sfx"], L["aglob"], rank, pairs_min=1, window_bits=4, **kw)
    after = hip_ctx.bwt_block(data, 8)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    for bad in (dict(pairs_min=0), dict(window_bits=0), dict(window_bits=33), dict(raw_out=True, text=False), dict(run_mode=1), dict(h_next=0)):
        with pytest.raises(hip.BwtcHipError) as e:
            hip_ctx.test_round(T, L["keys"], L["sfx"], L["aglob"], rank, **dict(dict(kw, pairs_min=L["m"], window_bits=16), **bad))
        assert e.value.code == -1, bad
