"""The 'B' coder's model passes on the GPU (wavelet_gpu_models.hip), pass by pass, against the sequential model
of tests/gmmodel.py on its hand-built cases (tests/test_gmmodel.py: the model against the product's sequential
host coder, every case against the edges it was built for).  bwtc_hip_test_models runs the product's own
wavelet_models_prepare / wavelet_models_run over a case's packed streams and tasks and copies back what every
pass left; all comparisons are equalities.

What each pass must leave is stated as a meaning: a chunk's map applied to every start state is the machines
walked over the chunk; the slot-space bits are the stable gather; a bracket resolved with its slot-chunk's true
start value is the true predictor value there.  Where the model's honest bracket is open at a border the
device's bracket there has that width and that base -- and is known exactly where the model says so."""
import numpy as np
import pytest

import gmmodel
from test_gmmodel import _invalid_inputs

pytestmark = pytest.mark.gpu
MAP_BITS = (1 << 38) - 1


def _popcount(v):
    v = np.asarray(v, np.uint64)
    return sum(((v >> np.uint64(i)) & np.uint64(1)) for i in range(32)).astype(np.int64)


def _resolve_all(x0, mask, L, t):
    """gmmodel.resolve over arrays; -1 where the true value lies outside an open bracket."""
    x0, mask, L, t = (np.asarray(a, np.int64) for a in (x0, mask, L, t))
    off = t - L
    ok = (mask == 0) | ((off >= 0) & (off <= 31))
    low = (np.int64(1) << np.clip(off, 0, 31)) - 1
    return np.where(ok, x0 + np.where(mask == 0, 0, _popcount(mask & low)), -1)


def _expected_maps(c, ex):
    """A chunk's map as the 38 bits mapApply reads: the machines walked over the chunk from every state.  (Each field is
    read by exactly one start state of its machine, so equal fields = equal images of all 8 x 4 x 3 packed states.)"""
    out = np.zeros(ex.nc, np.uint64)
    for i, (b, e, tf) in enumerate(ex.chunks.astype(np.int64).tolist()):
        m8, m4, m3 = gmmodel.machines_over(c.codes, b, e, int(c.tasks[tf & 0x7FFFFFFF, 2]))
        v = sum(m8[s] << (3 * s) for s in range(8)) | sum(m4[s] << (24 + 2 * s) for s in range(4)) | \
            sum(m3[s] << (32 + 2 * s) for s in range(3))
        out[i] = v
    return out


def _check_passes(c, r, state):
    name = c.name
    wk, ex = c.walk(state), c.expect(state)
    n, nc, nt, nsc = c.n, ex.nc, ex.nt, ex.nsc
    # chunks
    assert r["nc"] == nc and r["nsc"] == nsc, (name, r["nc"], nc)
    assert (r["chunks"] == ex.chunks).all(), name
    # pass 1: mapApply(cmap[c], s) over all packed start states = the machines walked over the chunk from s
    want = _expected_maps(c, ex)
    got = r["cmap"] & np.uint64(MAP_BITS)
    assert (got == want).all(), (name, "cmap", int(np.flatnonzero(got != want)[0]))
    for i in (0, nc // 2, nc - 1):                     # and literally, on three chunks
        b, e, tf = (int(x) for x in ex.chunks[i])
        m8, m4, m3 = gmmodel.machines_over(c.codes, b, e, int(c.tasks[tf & 0x7FFFFFFF, 2]))
        for s in (mc | gc << 3 | ic << 5 for mc in range(8) for gc in range(4) for ic in range(3)):
            assert gmmodel.map_apply(r["cmap"][i], s) == m8[s & 7] | m4[(s >> 3) & 3] << 3 | m3[s >> 5] << 5, (name, i, s)
    # the state scan
    assert (r["cstate"] == ex.cstate).all(), (name, "cstate", int(np.flatnonzero(r["cstate"] != ex.cstate)[0]))
    assert int(r["tail"][0]) == wk.state_out, name
    assert r["ends"].tolist() == gmmodel.end_states(c.codes, c.tasks), name
    # pass 2, the scan, the streams
    assert (r["base"] == ex.base).all(), (name, "base")
    assert (r["sb"] == ex.sb).all(), (name, "sb")
    assert int(r["base"][15 * nc]) == int(r["sb"][15 * nt]) == n == int(r["tail"][2]), name
    # pass 3
    assert r["sbits"].size == n // 32 + 16 and (r["sbits"] == ex.sbits).all(), (name, "sbits")
    # pass 5: the true value at every border.  One exception, by design: where a chain starts EXACTLY at the border the
    # slot-chunk starts from the slot's initial value, known without the walk (its brackets are closed throughout: checked
    # below, so nothing is ever resolved with sstart[j]); the walk hands on the end value of the chain before.
    want_start = ex.sstart.astype(np.int64)
    fresh = [j for j in range(1, nsc) if ex.chain_start_of(j * gmmodel.SLOT_CHUNK) == j * gmmodel.SLOT_CHUNK]
    for j in fresh:
        assert want_start[j] == gmmodel.slot_init(int(ex.slot_at[j * gmmodel.SLOT_CHUNK]))
        want_start[j] = ex.val_after[j * gmmodel.SLOT_CHUNK - 1]
        assert (r["snaps"][j * 64:(j + 1) * 64, 1] == 0).all(), (name, j, "a chunk that starts a chain has an open bracket")
    assert (r["sstart"] == want_start).all(), (name, "sstart", int(np.flatnonzero(r["sstart"] != want_start)[0]))
    # pass 4: the slot-chunks' maps, the brackets at the borders, the snapshots
    L = (r["smap"][:, 0] & 0xFFFF).astype(np.int64)
    x_end = (r["smap"][:, 0] >> 16).astype(np.int64)
    mask_end = r["smap"][:, 1].astype(np.int64)
    last = np.minimum((np.arange(nsc) + 1) * gmmodel.SLOT_CHUNK, n) - 1
    ends = _resolve_all(x_end, mask_end, L, r["sstart"])
    assert (ends == ex.val_after[last]).all(), (name, "slot-chunk end", int(np.flatnonzero(ends != ex.val_after[last])[0]))
    snap_x0 = r["snaps"][:, 0].astype(np.int64)
    snap_mask = r["snaps"][:, 1].astype(np.int64)
    for j in range(nsc):
        p0 = j * gmmodel.SLOT_CHUNK
        inside = ex.starts_inside(j)
        if inside:
            assert mask_end[j] == 0, (name, j)
        elif j + 1 < nsc and ex.chain_start_of(p0 + gmmodel.SLOT_CHUNK) <= p0:
            assert ends[j] == int(r["sstart"][j + 1]), (name, j)
        Lm, width = ex.bracket(j)
        assert L[j] == Lm and snap_x0[p0 // 32] == Lm, (name, j, int(L[j]), Lm)
        assert gmmodel.popcount(snap_mask[p0 // 32]) == width, (name, j, width)
        if width and not inside:
            img = ex.candidate_images(j)
            got_img = _resolve_all(np.full(width + 1, x_end[j]), np.full(width + 1, mask_end[j]), np.full(width + 1, Lm),
                                   Lm + np.arange(width + 1))
            assert (got_img == img).all(), (name, j, "candidates")
    pos = np.arange(0, n, gmmodel.SAMPLE)
    jc = pos // gmmodel.SLOT_CHUNK
    at = _resolve_all(snap_x0, snap_mask, L[jc], r["sstart"][jc].astype(np.int64))
    assert (at == ex.val[pos]).all(), (name, "snapshot", int(pos[np.flatnonzero(at != ex.val[pos])[0]]))
    # pass 7
    assert int(r["tail"][1]) == 0 and int(r["tail"][3]) == 0, (name, r["tail"])
    assert (r["w"] == wk.w).all(), (name, "w", int(np.flatnonzero(r["w"] != wk.w)[0]))


@pytest.mark.parametrize("name", gmmodel.CASE_NAMES)
def test_model_passes_match_the_model(name, hip_ctx):
    c = gmmodel.case(name)
    r = hip_ctx.test_models(c.packed, c.n, c.tasks, c.state_in)
    _check_passes(c, r, c.state_in)


@pytest.mark.parametrize("name", gmmodel.CASE_NAMES)
def test_lines_form_leaves_the_same(name, hip_ctx):
    """k_gm_partition_lines (flags bit 0) in place of k_gm_partition: w and every intermediate identical."""
    c = gmmodel.case(name)
    a = hip_ctx.test_models(c.packed, c.n, c.tasks, c.state_in)
    b = hip_ctx.test_models(c.packed, c.n, c.tasks, c.state_in, flags=1)
    assert (b["sbits"] == c.expect().sbits).all(), name
    for k in sorted(a):
        assert np.array_equal(a[k], b[k]), (name, k)
    assert (b["w"] == c.walk().w).all(), name


@pytest.mark.parametrize("name", gmmodel.SCAN_CASES)
def test_state_scan_from_every_start_state(name, hip_ctx):
    """cstate, tail[0] and w from each of the eight states the block can start in (flags bit 1 would skip cstate)."""
    c = gmmodel.case(name)
    for s in range(8):
        wk, ex = c.walk(s), c.expect(s)
        r = hip_ctx.test_models(c.packed, c.n, c.tasks, s)
        assert (r["cstate"] == ex.cstate).all(), (name, s)
        assert int(r["tail"][0]) == wk.state_out and int(r["ends"][s]) == wk.state_out, (name, s)
        assert (r["w"] == wk.w).all() and int(r["tail"][1]) == 0, (name, s)
        lean = hip_ctx.test_models(c.packed, c.n, c.tasks, s, flags=2)
        assert (lean["w"] == wk.w).all() and lean["tail"].tolist() == r["tail"].tolist(), (name, s)


@pytest.mark.parametrize("name", ["streams_nc273", "streams_nc274", "total_65541"])
def test_slot_base_scan_in_the_chained_form(name, monkeypatch):
    """The slot-base scan (15 nc + 1 words: one tile at nc = 273, two at 274) on a fresh context whose scans take the
    single-launch chained form."""
    from bwtc_amd import hip
    monkeypatch.setenv("BWTC_HIP_SCAN", "chained")
    c = gmmodel.case(name)
    with hip.Context(0, 1 << 20) as ctx:
        r = ctx.test_models(c.packed, c.n, c.tasks, c.state_in)
    _check_passes(c, r, c.state_in)


def test_refusals_launch_nothing_and_leave_the_context_usable(hip_ctx):
    from bwtc_amd import hip
    c = gmmodel.case("tiny_ladder")
    for packed, n, tasks, state in _invalid_inputs(c):
        with pytest.raises(hip.BwtcHipError) as e:
            hip_ctx.test_models(packed, n, tasks, state)
        assert e.value.code == -1
    # more elements than the context's workspace holds (nothing of `packed` is read before the refusal)
    with pytest.raises(hip.BwtcHipError) as e:
        hip_ctx.test_models(c.packed, 0xFFFFF000, np.array([[0, 0xFFFFF000, 0]], np.uint32), 0, flags=2)
    assert e.value.code == -1
    # null arguments, no elements, no tasks, unknown flags
    L, h, o = hip_ctx.lib, hip_ctx.handle, hip.ModelsOut()
    w = np.zeros(c.n, np.uint16)
    o.w = hip._ptr(w)
    import ctypes
    pk, tk, nt = hip._ptr(c.packed), hip._ptr(c.tasks), c.tasks.shape[0]
    assert L.bwtc_hip_test_models(None, pk, c.n, tk, nt, 0, 2, ctypes.byref(o)) == -1
    assert L.bwtc_hip_test_models(h, None, c.n, tk, nt, 0, 2, ctypes.byref(o)) == -1
    assert L.bwtc_hip_test_models(h, pk, c.n, None, nt, 0, 2, ctypes.byref(o)) == -1
    assert L.bwtc_hip_test_models(h, pk, c.n, tk, nt, 0, 2, None) == -1
    assert L.bwtc_hip_test_models(h, pk, 0, tk, nt, 0, 2, ctypes.byref(o)) == -1
    assert L.bwtc_hip_test_models(h, pk, c.n, tk, 0, 0, 2, ctypes.byref(o)) == -1
    assert L.bwtc_hip_test_models(h, pk, c.n, tk, nt, 0, 4, ctypes.byref(o)) == -1
    assert L.bwtc_hip_test_models(h, pk, c.n, tk, nt, 0, 0, ctypes.byref(o)) == -1      # the intermediates' room is missing
    r = hip_ctx.test_models(c.packed, c.n, c.tasks, c.state_in)
    _check_passes(c, r, c.state_in)
