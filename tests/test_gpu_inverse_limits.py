"""GPU tests of the inverse transform at its limits (bwtc_hip_inverse_bwt_block / _device, inverse_bwt.hip).

The transformed bytes and the LF powers come from the ORACLE's forward transform, never from the GPU's own; the
expected bytes are the input block; every comparison is exact; every accepted call leaves stats().n == size + 1,
read after a call on a block of another size, so that a stale value cannot pass.  Refused and damaged inputs are held
to tests/invmodel.py, which says for any input what the inverse must do: the model's bytes, or its return code.

Sizes sit on the boundaries of the code (n = size + 1 rows): one splitter (n <= 64), two, a splitter count one below,
at and above a power of two (the rounds of pointer jumping), the 512-row wave segment and the 4096-row tile of
k_inv_hist / k_inv_lf, and 16 -> 17 tiles, where the scan of the tile histograms leaves its one-workgroup form
(ntiles * 256 > 4096).  End-of-block rows are placed on row 1, on `size` (the row whose character is bwt[size]), on
splitter rows and on tile edges.

Not here: the scan's second look-back stride needs more than 16 Mi rows, and the oracle's forward transform takes
about ten seconds for 16 MiB; the 64 MiB and 1 GiB round trips of test_gpu_inverse.py and test_gpu_bwt.py keep
covering it."""
import ctypes

import numpy as np
import pytest

import invmodel

pytestmark = pytest.mark.gpu
GUARD = 64
PAD = 0xA5
BIG = invmodel.SIZES[-1]
PARAMS = [(s, tuple(invmodel.block_names(s))) for s in invmodel.SIZES[:-1]] + [(BIG, (k,)) for k in invmodel.block_names(BIG)]
_vp = ctypes.c_void_p
_cache = {}


def _ids(p):
    return "%d-%s" % (p[0], p[1][0] if len(p[1]) == 1 else "all")


def _shared(oracle, size, name):
    """(block, oracle's bwt, oracle's LF powers) of a shared block, computed once."""
    key = (size, name)
    if key not in _cache:
        d = invmodel.block(size, name)
        bwt, lf, _ = oracle.oracle_bwt_block(d, invmodel.starting_points(size, name))
        d.setflags(write=False); bwt.setflags(write=False); lf.setflags(write=False)
        _cache[key] = (d, bwt, lf)
    return _cache[key]


def _forward(oracle, d, sp):
    bwt, lf, _ = oracle.oracle_bwt_block(d, sp)
    return bwt, lf


def _host(ctx, bwt, lf, n_lf=None):
    """The host entry on a caller's block of size + 1 bytes: (return code, the block's first size bytes).  The byte
    after the block keeps its value, as the header promises."""
    size = int(bwt.size)
    buf = np.empty(size + 1, np.uint8)
    buf[:size] = bwt
    buf[size] = PAD
    lfa = np.ascontiguousarray(lf, np.uint32)
    rc = ctx.lib.bwtc_hip_inverse_bwt_block(ctx.handle, buf.ctypes.data_as(_vp), size, lfa.ctypes.data_as(_vp),
                                            lfa.size if n_lf is None else n_lf)
    assert buf[size] == PAD, "the byte after the block was written"
    return rc, buf[:size]


def _other_size_first(ctx, size):
    """Makes stats().n differ from size + 1 by an all-equal block of another size; returns the value."""
    if ctx.stats().n == size + 1:
        k = 5 if size != 5 else 6
        rc, _ = _host(ctx, np.full(k, 9, np.uint8), [k])
        assert rc == 0
    before = ctx.stats().n
    assert before != size + 1
    return before


def _accepted(ctx, bwt, lf, want, what):
    _other_size_first(ctx, bwt.size)
    rc, got = _host(ctx, bwt, lf)
    assert rc == 0, (what, rc)
    assert got.tobytes() == want.tobytes(), what
    assert ctx.stats().n == bwt.size + 1, what


def _refused(ctx, bwt, lf, code, what, n_lf=None):
    rc, got = _host(ctx, bwt, lf, n_lf)
    assert rc == code, (what, rc, code)
    assert got.tobytes() == np.asarray(bwt, np.uint8).tobytes(), (what, "a refused block was changed")


def _as_the_model_says(ctx, bwt, lf, what):
    m = invmodel.lf_model(bwt, lf)
    if m.rc == 0:
        _accepted(ctx, bwt, lf, m.out, what)
    else:
        _refused(ctx, bwt, lf, m.rc, what)
    return m


# ---- sizes, contents, end-of-block rows ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", PARAMS, ids=_ids)
def test_sizes_contents_and_end_of_block_rows(hip_ctx, oracle, case):
    size, names = case
    for name in names:
        d, bwt, lf = _shared(oracle, size, name)
        if name.startswith("eob_"):
            assert int(lf[0]) == int(name[4:])
        if name == "all_equal":
            assert int(lf[0]) == size
        _accepted(hip_ctx, bwt, lf, d, (size, name, lf.size))


# ---- LF powers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", invmodel.POWER_SIZES)
def test_every_count_of_lf_powers_with_a_remainder(hip_ctx, oracle, size):
    n = size + 1
    blocks = invmodel.power_blocks(size)
    assert tuple(k for k, _ in blocks) == invmodel.N_LFS
    for n_lf, d in blocks:
        assert n_lf == 1 or n % n_lf != 0
        bwt, lf = _forward(oracle, d, n_lf)
        assert lf.size == n_lf
        _accepted(hip_ctx, bwt, lf, d, (size, n_lf))


def test_a_power_after_the_last_splitter_of_the_walk(hip_ctx, oracle):
    """x = 1: the check's way from such a power to a splitter ends at row 0, index 0 of the walk, and the power's own
    index is n - steps."""
    d, bwt, lf, ks = invmodel.wrap_case(lambda data, sp: _forward(oracle, data, sp))
    m = invmodel.lf_model(bwt, lf)
    last = int(m.pos[::invmodel.SPLIT].max())
    assert len(ks) >= 2 and all(int(m.pos[int(lf[k])]) > last for k in ks)
    _accepted(hip_ctx, bwt, lf, d, "wrap")
    for k in ks:
        for delta in (-1, 1):
            bad = lf.copy()
            bad[k] = int(lf[k]) + delta
            if 0 <= int(bad[k]) <= d.size:
                assert invmodel.lf_model(bwt, bad).rc == -4
                _refused(hip_ctx, bwt, bad, -4, ("wrap", k, delta))


@pytest.mark.parametrize("size,n_lf", invmodel.OFF_BY_ONE)
def test_every_power_off_by_one_is_refused(hip_ctx, oracle, size, n_lf):
    d = invmodel.plain_block(size, n_lf)
    bwt, lf = _forward(oracle, d, n_lf)
    assert lf.size == n_lf
    _accepted(hip_ctx, bwt, lf, d, (size, n_lf))
    tried = 0
    for k in range(1, n_lf):
        for delta in (-1, 1):
            v = int(lf[k]) + delta
            if 0 <= v <= size:
                bad = lf.copy()
                bad[k] = v
                _refused(hip_ctx, bwt, bad, -4, (size, n_lf, k, delta))     # LF is one cycle: no other row is at that index
                tried += 1
    assert tried >= 2 * (n_lf - 1) - 2
    bad = lf.copy()
    bad[1], bad[2] = lf[2], lf[1]
    _refused(hip_ctx, bwt, bad, -4, "powers 1 and 2 swapped")
    for k in (1, n_lf - 1):
        bad = lf.copy()
        bad[k] = size + 1
        _refused(hip_ctx, bwt, bad, -4, "a power that is no row")
    _accepted(hip_ctx, bwt, lf, d, "after the refusals")


def test_arguments_and_more_powers_than_rows(hip_ctx, oracle):
    d = invmodel.block(510, "random256")
    bwt, lf = _forward(oracle, d, 8)
    bad = lf.copy()
    bad[0] = d.size + 1
    _refused(hip_ctx, bwt, bad, -1, "end-of-block row outside the block")
    _refused(hip_ctx, bwt, lf, -1, "no powers", n_lf=0)
    _refused(hip_ctx, bwt, np.concatenate([lf, np.zeros(249, np.uint32)]), -1, "257 powers")
    for code, powers in ((-1, [d.size + 1]), (-1, []), (-1, [0] * 257), (-4, [int(lf[0]), d.size + 1])):
        assert invmodel.lf_model(bwt, powers).rc == code
    d5 = invmodel.block_with_eob(5, 3, np.random.default_rng(1))
    b5, l5 = _forward(oracle, d5, 1)
    _accepted(hip_ctx, b5, l5, d5, "5 bytes")
    for fill in (0, 3, 5):
        many = np.array([int(l5[0])] + [fill] * 255, np.uint32)          # x = 6 / 256 = 0: index k * x - 1 does not exist
        m = _as_the_model_says(hip_ctx, b5, many, ("256 powers on 5 bytes", fill))
        assert m.rc == -4 and m.one_cycle


# ---- damaged input -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", invmodel.DAMAGE_SIZES)
def test_damaged_input_does_what_the_model_says(hip_ctx, oracle, size):
    d = invmodel.block(size, "random2" if size == 4096 else "random256")
    for sp in (8, 1):
        bwt, lf = _forward(oracle, d, sp)
        _accepted(hip_ctx, bwt, lf, d, (size, sp))
        two = invmodel.damage_two_cycles(bwt, lf)
        m = _as_the_model_says(hip_ctx, two, lf, (size, sp, "two cycles"))
        assert m.rc == -4 and invmodel.cycles_without_splitter(m.LF)[0] == 2
        lone = invmodel.damage_cycle_without_splitter(bwt, lf)
        m = _as_the_model_says(hip_ctx, lone, lf, (size, sp, "a cycle without a splitter row"))
        assert m.rc == -4 and invmodel.cycles_without_splitter(m.LF) == (2, 1)
        one = invmodel.damage_one_cycle(bwt, lf)
        m = _as_the_model_says(hip_ctx, one, lf, (size, sp, "one cycle again"))
        assert m.one_cycle and (sp != 1 or (m.rc == 0 and m.out.tobytes() != d.tobytes()))
        hurt = bwt.copy()
        hurt[size // 3:size // 3 + 10] ^= 0x55
        _as_the_model_says(hip_ctx, hurt, lf, (size, sp, "ten bytes changed"))
        for eob in (1, size, (int(lf[0]) + 777) % size + 1, int(lf[0]) + 1, int(lf[0]) - 1):
            if 0 <= eob <= size:
                moved = lf.copy()
                moved[0] = eob
                _as_the_model_says(hip_ctx, bwt, moved, (size, sp, "end-of-block row moved to", eob))
        _accepted(hip_ctx, bwt, lf, d, (size, sp, "afterwards"))


# ---- memory ------------------------------------------------------------------------------------------------------------
class _Guarded:
    """Device memory with `span` bytes at `offset` from a 256-byte boundary, 0xA5 all around."""

    def __init__(self, ctx, span, offset):
        self.ctx, self.span, self.room = ctx, span, 256 + offset + span + GUARD
        self.raw = ctx.lib.bwtc_hip_malloc(ctx.handle, self.room + 256)
        assert self.raw
        self.base = (self.raw + 255) // 256 * 256
        self.at = self.base + 256 + offset
        self.lead = 256 + offset
        fill = np.full(self.room, PAD, np.uint8)
        assert ctx.lib.bwtc_hip_memcpy_to_device(ctx.handle, self.base, fill.ctypes.data, self.room) == 0

    def put(self, data):
        data = np.ascontiguousarray(data, np.uint8)
        assert self.ctx.lib.bwtc_hip_memcpy_to_device(self.ctx.handle, self.at, data.ctypes.data, data.size) == 0

    def get(self):
        """(the span's bytes, guards intact)"""
        back = np.empty(self.room, np.uint8)
        assert self.ctx.lib.bwtc_hip_memcpy_to_host(self.ctx.handle, back.ctypes.data, self.base, self.room) == 0
        intact = (back[:self.lead] == PAD).all() and (back[self.lead + self.span:] == PAD).all()
        return back[self.lead:self.lead + self.span].copy(), bool(intact)

    def free(self):
        self.ctx.lib.bwtc_hip_free(self.ctx.handle, self.raw)


def _device(ctx, bwt, lf, offset, mode):
    """The device entry inside guards: (return code, what d_out holds, d_bwt's buffer afterwards, guards intact)."""
    size = int(bwt.size)
    lfa = np.ascontiguousarray(lf, np.uint32)
    a = _Guarded(ctx, size + (1 if mode == "shifted" else 0), offset)
    b = _Guarded(ctx, size, offset) if mode == "disjoint" else None
    try:
        a.put(bwt)
        d_out = b.at if b else a.at + (1 if mode == "shifted" else 0)
        rc = ctx.lib.bwtc_hip_inverse_bwt_block_device(ctx.handle, _vp(a.at), _vp(d_out), size, lfa.ctypes.data_as(_vp), lfa.size)
        src, ok_a = a.get()
        if b:
            out, ok_b = b.get()
        else:
            out, ok_b = (src[1:] if mode == "shifted" else src), True
        return rc, out, src, ok_a and ok_b
    finally:
        a.free()
        if b:
            b.free()


@pytest.mark.parametrize("size", (1, 63, 4096, 65536))
def test_device_entry_inside_guards(hip_ctx, oracle, size):
    for name in ("all_equal", "random256"):                 # all_equal: the end-of-block row is `size`
        d, bwt, lf = _shared(oracle, size, name)
        bad = None
        if lf.size > 1:
            bad = lf.copy()
            bad[1] = (int(lf[1]) + 1) % (size + 1)
        for offset in (0, 1, 7, 15):
            for mode in ("disjoint", "same", "shifted"):
                what = (size, name, offset, mode)
                _other_size_first(hip_ctx, size)
                rc, out, src, intact = _device(hip_ctx, bwt, lf, offset, mode)
                assert rc == 0 and intact, what
                assert out.tobytes() == d.tobytes(), what
                assert hip_ctx.stats().n == size + 1
                if mode == "disjoint":
                    assert src.tobytes() == bwt.tobytes(), what
                if mode == "shifted":
                    assert src[0] == bwt[0], what
                if bad is not None:
                    rc, _, src, intact = _device(hip_ctx, bwt, bad, offset, mode)
                    assert rc == -4 and intact, what
                    if mode == "disjoint":
                        assert src.tobytes() == bwt.tobytes(), what
    # a block that is refused for its cycles, not for a power
    d, bwt, lf = _shared(oracle, 65536, "random256")
    two = invmodel.damage_two_cycles(bwt, lf)
    for mode in ("disjoint", "same", "shifted"):
        rc, _, _, intact = _device(hip_ctx, two, lf, 7, mode)
        assert rc == -4 and intact, mode


# ---- one context, many calls ---------------------------------------------------------------------------------------------
def test_one_context_many_calls(hip_ctx, oracle):
    """Large, one byte, refused, 65536, 63 on the shared context: no word of a larger call (len, nxt, dist, the table,
    the check's verdict) may reach a later one."""
    big = _shared(oracle, BIG, "random256")
    one = _shared(oracle, 1, "random256")
    mid = _shared(oracle, 65536, "random2")
    small = _shared(oracle, 63, "eob_63")
    _accepted(hip_ctx, big[1], big[2], big[0], "large")
    assert hip_ctx.stats().n == BIG + 1
    _accepted(hip_ctx, one[1], one[2], one[0], "one byte")
    two = invmodel.damage_two_cycles(mid[1], mid[2])
    assert invmodel.lf_model(two, mid[2]).rc == -4
    _refused(hip_ctx, two, mid[2], -4, "two cycles")
    _accepted(hip_ctx, mid[1], mid[2], mid[0], "65536")
    _accepted(hip_ctx, small[1], small[2], small[0], "63")
    _accepted(hip_ctx, big[1], big[2], big[0], "large again")
