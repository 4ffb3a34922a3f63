"""The GPU radix sorts (bwtc_amd/csrc/radix_sort.hpp) at their tile, digit, hole and key-word limits, each form called on
its own through the hooks bwtc_hip_test_radix_* and held to tests/sortmodel.py by exact equality: keys, values and
second words.  The named cases and their inputs are sortmodel.cases() / make(); tests/test_sortmodel.py shows the model
equal to brute force and every case at the edge it is named for.  The hooks check the sorts' contracts on the host,
make the producer's first digit plane themselves and guard every buffer with canaries (a changed one raises)."""
import numpy as np
import pytest

import sortmodel as sm
from bwtc_amd import hip

pytestmark = pytest.mark.gpu


def _run(ctx, c):
    inp = sm.make(c)
    want = sm.expected(c, inp)
    if c["form"] == "plain":
        gk, gv = ctx.test_radix_pairs(inp["keys"], inp.get("vals"), n_holes=c["n_holes"], bit_lo=c["bit_lo"], nbits=c["nbits"],
                                      values=c["values"], planes=c["planes"], vtype=sm.DT[c["vtype"]])
        assert gk.size == c["n"] and np.array_equal(gk, want[0]), c["name"]
        if c["values"] == "keys":
            assert gv is None
        else:
            assert gv.dtype == sm.DT[c["vtype"]] and np.array_equal(gv, want[1]), c["name"]
    elif c["form"] == "long":
        gk, gv, gw = ctx.test_radix_long(inp["keys"], inp["w"], c["kbits"], c["wbits"], vtype=sm.DT[c["vtype"]], items_per_thread=c["el"],
                                         direct_w=bool(c["direct_w"]))
        assert np.array_equal(gk, want[0]), c["name"]           # the payload above kbits came back with its item
        assert np.array_equal(gw, want[2]), c["name"]
        assert gv.dtype == sm.DT[c["vtype"]] and np.array_equal(gv, want[1]), c["name"]
    else:
        got = ctx.test_radix_segmented(inp["keys"], c["bit_lo"], inp["tile_first"])
        assert np.array_equal(got, want), c["name"]


def _bucket(ctx, group, bucket):
    cs = [c for c in sm.cases(group) if c["bucket"] == bucket]
    assert cs
    for c in cs:
        _run(ctx, c)


@pytest.mark.parametrize("bucket", sm.buckets("seams"))
def test_tile_seams(hip_ctx, bucket):
    """Plain sort, n = t * TILE + d for t in {1, 2, 7, 8, 9, 16, 17}, d in {-1, 0, +1}, and n in {1, 2, 63, 64, 65}; both
    key types, planes on and off, nbits from one bit to the whole key (a top digit of 1..8 bits).  The tile-to-XCD dealing
    tile = (blockIdx & 7) * per_xcd + (blockIdx >> 3) with unused slots, the odd tile of k_radix_hist_plane's pairs and
    its partial-load path, and the offset table's scan by one workgroup (up to 16 tiles) or three launches (17)."""
    _bucket(hip_ctx, "seams", bucket)


@pytest.mark.parametrize("bucket", sm.buckets("digits"))
def test_digit_shapes(hip_ctx, bucket):
    """Plain sort at one tile + 1 and nine tiles - 1: every item the same digit in every pass, two digits alternating lane
    by lane, digits 0 and 255 only, every digit value n / 256 times, one hot digit with 99 % of the items, and the
    all-ones key as an item (no hole mode: it sorts last).  The wave ballots' ranks, the per-wave counters s_cnt[wave][d]
    and the interleaved histogram copies at their most and least crowded."""
    _bucket(hip_ctx, "digits", bucket)


@pytest.mark.parametrize("bucket", sm.buckets("payload"))
def test_payload_beside_the_sorted_field(hip_ctx, bucket):
    """A sorted field that does not start at bit 0 (bit_lo in {8, 12, 32, 40}, random bits below it: scatter_rank_pairs'
    partition by the top bits of a 32-bit destination), the window
    partition of records in its shape nbits = 32 + bits, bit_lo = 32 + lo with the first plane ready (plane0_ready: the first histogram
    comes from a plane the sort did not write), and u64 keys with random bits 56..63: the order ignores the payload,
    ties keep their input order, every bit comes back unchanged."""
    _bucket(hip_ctx, "payload", bucket)


@pytest.mark.parametrize("bucket", sm.buckets("values"))
def test_values_the_first_pass_makes_up(hip_ctx, bucket):
    """values_mode 1 (positions) and 3 (descending slots) on the first pass, keys-only sorts (KEYS; for u32 in the step
    sort's shape, the field from kStepLeafShift with the plane ready) and 16-bit values (V = unsigned short), at 1, 2 and 9
    tiles +- 1, planes off and on with the first plane ready."""
    _bucket(hip_ctx, "values", bucket)


@pytest.mark.parametrize("bucket", sm.buckets("holes"))
def test_holes(hip_ctx, bucket):
    """n_holes > 0, the SKIP instantiations of k_radix_hist / k_radix_scatter (the compacting first pass): n_holes in
    {1, TILE - 1, TILE, n} around 1, 2 and 9 tiles; holes all in one tile, a tile of nothing but holes, holes only at the
    end, holes at every other slot; n = 1 with holes; nbits = 0 (one compacting pass, order kept).  Planes on and off:
    with planes the first pass reads the keys although a plane exists, and leaves the second pass's plane."""
    _bucket(hip_ctx, "holes", bucket)


@pytest.mark.parametrize("bucket", sm.buckets("long"))
def test_long_sort(hip_ctx, bucket):
    """radix_sort_long in the three instantiations <u32, 6>, <u16, 6>, <u16, 8>, direct_w on (k_radix_hist_words) and off
    (k_radix_hist_plane), at 1, 2, 9 and 17 long tiles +- 1: passes over w first, then the bridge digit when wbits % 8 != 0,
    then the key's with the top-digit mask dmask.  (kbits, wbits) = (40, 32) no bridge, (33, 21) a bridge of 5 bits,
    (17, 7) and (9, 4) start with the bridge, (3, 4) and (1, 1) are one masked digit, (64, 32) no payload room, (48, 16);
    random payload above kbits; the -few buckets have ties that span tiles."""
    _bucket(hip_ctx, "long", bucket)


@pytest.mark.parametrize("bucket", sm.buckets("seg"))
def test_segmented_sort(hip_ctx, bucket):
    """radix_sort_keys_segmented: the SEG table layout (seg_table_at), seg_of_tile over empty segments (first, last, in
    the middle, several in a row) and the all-ones padding; 1, 2 and 256 segments of 1, 2 and 9 tiles, a segment that is
    all padding but for one key, real keys whose field is 0xFFFF next to the padding, bit_lo in {0, kStepLeafShift}; the
    other bits are random and come back unchanged, in stable order."""
    _bucket(hip_ctx, "seg", bucket)


def _refused(call):
    with pytest.raises(hip.BwtcHipError) as e:
        call()
    return e.value.code


def test_contract_refusals(hip_ctx):
    """Host checks of the hooks: nothing malformed is launched (-1), and the context still sorts afterwards."""
    T = sm.TILE["u32"]
    rng = np.random.default_rng(1)
    k = rng.integers(0, 1 << 32, 3 * T, dtype=np.uint64).astype(np.uint32)
    k[k == 0xFFFFFFFF] = 0
    v = np.arange(k.size, dtype=np.uint32)
    holes = k.copy()
    holes[5::97] = 0xFFFFFFFF
    h = int((holes == 0xFFFFFFFF).sum())
    assert _refused(lambda: hip_ctx.test_radix_pairs(holes, v, n_holes=h - 1)) == -1            # a wrong hole count
    assert _refused(lambda: hip_ctx.test_radix_pairs(holes, v, n_holes=h + 1)) == -1
    assert _refused(lambda: hip_ctx.test_radix_pairs(k, v, n_holes=1)) == -1
    assert _refused(lambda: hip_ctx.test_radix_pairs(k, v, bit_lo=9, nbits=8)) == -1            # bit_lo <= nbits <= 8 * sizeof(K)
    assert _refused(lambda: hip_ctx.test_radix_pairs(k, v, nbits=33)) == -1
    assert _refused(lambda: hip_ctx.test_radix_pairs(holes, n_holes=h, values="descending")) == -1
    assert _refused(lambda: hip_ctx.test_radix_pairs(k[:1], values="positions")) == -1          # no pass would make the values
    assert _refused(lambda: hip_ctx.test_radix_pairs(np.zeros((64 << 20) + 1024, np.uint32), values="keys")) == -1   # does not fit
    tf = np.array([0, 1, 3], np.uint32)
    assert _refused(lambda: hip_ctx.test_radix_segmented(k, 0, [0, 1, 2])) == -1                # does not end at the tile count
    assert _refused(lambda: hip_ctx.test_radix_segmented(k, 0, [1, 2, 3])) == -1
    assert _refused(lambda: hip_ctx.test_radix_segmented(k, 0, [0, 2, 1, 3])) == -1
    assert _refused(lambda: hip_ctx.test_radix_segmented(k[:-1], 0, tf)) == -1                  # whole tiles only
    assert _refused(lambda: hip_ctx.test_radix_segmented(k, 17, tf)) == -1
    k64 = k.astype(np.uint64)
    assert _refused(lambda: hip_ctx.test_radix_long(k64, k, 40, 21)) == -1                      # w has bits at or above wbits
    assert _refused(lambda: hip_ctx.test_radix_long(k64, k, 65, 32)) == -1
    assert _refused(lambda: hip_ctx.test_radix_long(k64, k, 40, 32, vtype=np.uint32, items_per_thread=8)) == -1   # no such instantiation
    # and the context still sorts
    gk, gv = hip_ctx.test_radix_pairs(holes, v, n_holes=h)
    wk, wv = sm.plain_expected(holes, v, h)
    assert np.array_equal(gk, wk) and np.array_equal(gv, wv)
    assert np.array_equal(hip_ctx.test_radix_segmented(k, 0, tf), sm.seg_expected(k, 0, tf))
    gk, gv, gw = hip_ctx.test_radix_long(k64, k, 40, 32)
    wk, wv, ww = sm.long_expected(k64, k, 40, 32)
    assert np.array_equal(gk, wk) and np.array_equal(gv, wv) and np.array_equal(gw, ww)
