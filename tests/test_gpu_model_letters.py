"""The model passes of the coders 'b' and 'u' on the GPU (the letter instantiations of wavelet_gpu_models.hip) against
the sequential walk of tests/lettermodel.py (tests/test_lettermodel.py: the walk against the product's sequential host
coder, every case against what it was built for).  bwtc_hip_test_models_letter runs the product's own
wavelet_models_prepare / wavelet_models_run with the letter's kind over a case's packed streams and tasks; all
comparisons are equalities: w, the chunks' start states, the tail words (no flag, every element counted, the state
handed on) and ends, in both forms of the partition pass and in the lean form."""
import numpy as np
import pytest

import gmmodel
import lettermodel

pytestmark = pytest.mark.gpu
LETTERS = lettermodel.LETTERS


@pytest.fixture(scope="module")
def ctx():
    from bwtc_amd import hip
    with hip.Context(0, 1 << 20) as c:
        yield c


def _check(c, letter, name, r, lean=False):
    wk = lettermodel.case_walk(letter, name)
    assert (r["w"] == wk.w).all(), (name, letter, "w", int(np.flatnonzero(r["w"] != wk.w)[0]))
    assert r["tail"].tolist() == [lettermodel.MAIN_START[letter], 0, c.n, 0], (name, letter, r["tail"])
    assert r["ends"].tolist() == list(range(8)), (name, letter)
    if lean:
        return
    chunks, _ = gmmodel.cut_chunks(c.tasks)
    assert r["nc"] == chunks.shape[0] and (r["chunks"] == chunks).all(), (name, letter)
    want = wk.states[chunks[:, 0].astype(np.int64)]
    assert (r["cstate"] == want).all(), (name, letter, "cstate", int(np.flatnonzero(r["cstate"] != want)[0]))
    assert int(r["base"][15 * r["nc"]]) == c.n


@pytest.mark.parametrize("letter", LETTERS)
@pytest.mark.parametrize("name", lettermodel.CASE_NAMES)
def test_letter_passes_match_the_walk(name, letter, ctx):
    c = lettermodel.case(name)
    r = ctx.test_models(c.packed, c.n, c.tasks, c.state_in, letter=letter)
    _check(c, letter, name, r)
    lines = ctx.test_models(c.packed, c.n, c.tasks, c.state_in, flags=1, letter=letter)
    _check(c, letter, name, lines)
    for k in sorted(r):
        assert np.array_equal(r[k], lines[k]), (name, letter, k)
    lean = ctx.test_models(c.packed, c.n, c.tasks, c.state_in, flags=2, letter=letter)
    _check(c, letter, name, lean, lean=True)


@pytest.mark.parametrize("letter", LETTERS)
@pytest.mark.parametrize("name", ["tiny_ladder", "meet_grid", "period6", "alt_from_1", "scan_nc8193"])
def test_the_carried_state_changes_nothing(name, letter, ctx):
    c = lettermodel.case(name)
    a = ctx.test_models(c.packed, c.n, c.tasks, 0, letter=letter)
    b = ctx.test_models(c.packed, c.n, c.tasks, 7, letter=letter)
    _check(c, letter, name, a)
    for k in sorted(a):
        assert np.array_equal(a[k], b[k]), (name, letter, k)


def test_letter_passes_raise_no_flag_where_two_values_stay_apart(ctx):
    """Main slots carry their three candidates exactly: under alternating bits two stay apart across every slot-chunk and
    chain-group border (tests/test_lettermodel.py), the slot-chunks' maps say so, and no error flag is raised."""
    c = lettermodel.case("alt_from_0")
    r = ctx.test_models(c.packed, c.n, c.tasks, 0, letter="u")
    assert r["nsc"] == 20 and int(r["tail"][1]) == 0
    assert (r["smap"][1:, 1] != 0).all()                       # every later slot-chunk ends with two candidates apart
    wk = lettermodel.case_walk("u", "alt_from_0")
    assert (r["sstart"].astype(np.int64) == wk.before[::gmmodel.SLOT_CHUNK] // 1024 - 1).all()


def test_letter_hook_refuses_other_letters_and_keeps_B(ctx):
    from bwtc_amd import hip
    c = lettermodel.case("tiny_ladder")
    for letter in ("m", "H", "x"):
        with pytest.raises(hip.BwtcHipError) as e:
            ctx.test_models(c.packed, c.n, c.tasks, 0, flags=2, letter=letter)
        assert e.value.code == -1
    o = hip.ModelsOut()
    w = np.zeros(c.n, np.uint16)
    o.w = hip._ptr(w)
    import ctypes
    rc = ctx.lib.bwtc_hip_test_models_letter(ctx.handle, b"B", hip._ptr(c.packed), c.n, hip._ptr(c.tasks), c.tasks.shape[0], c.state_in, 2,
                                             ctypes.byref(o))
    assert rc == 0 and (w == c.walk().w).all() and int(o.tail[0]) == c.walk().state_out
