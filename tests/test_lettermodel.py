"""CPU tests of tests/lettermodel.py -- the sequential walk the GPU models of the coders 'b' and 'u' are held to in
tests/test_gpu_model_letters.py -- and of the letters' passes run lane by lane on the host.

The anchor: the walk's w equals the w of the product's SEQUENTIAL host coder under the letter (StreamCoder::model,
bwtc_hip_host_wavelet_elements_letter) on real sections of text, DNA, random and all-equal blocks; that coder's bytes
are held equal to the oracle's in tests/test_host_logic.py.  Then: the host lanes (bwtc_hip_host_test_models_letter)
give the walk's w on every case, every case tells a letter from 'B', and every named case is what its name says --
shown with the walk alone."""
import numpy as np
import pytest

import blockgen
import gmmodel
import lettermodel
from gmmodel import CHUNK, INNER, ROOT, SLOT_CHUNK
from test_gmmodel import _section_args

LETTERS = lettermodel.LETTERS


def _real_blocks():
    """Text, DNA, random and all-equal blocks of blockgen.structured, 200 KiB each."""
    rng = np.random.default_rng(77)
    want, out = {5: "text", 6: "dna", 3: "random", 0: "all_equal"}, {}
    while len(out) < len(want):
        kind, d = blockgen.structured(rng, 200 << 10)
        if kind in want and want[kind] not in out:
            out[want[kind]] = d
    return out


@pytest.fixture(scope="module")
def real_elements(oracle):
    """name -> the section-run arguments of the block's transform."""
    args = {}
    for name, d in _real_blocks().items():
        bwt, _, freqs = oracle.oracle_bwt_block(d, 4)
        args[name] = _section_args(bwt, oracle.oracle_sections(freqs))
    return args


@pytest.mark.parametrize("letter", LETTERS)
@pytest.mark.parametrize("name", ["text", "dna", "random", "all_equal"])
def test_walk_matches_the_sequential_host_coder(name, letter, real_elements):
    from bwtc_amd import hip
    args = real_elements[name]
    packed, n, tasks, w, end = hip.host_wavelet_elements(args, 5, letter=letter)
    assert n > 0
    codes = gmmodel.unpack_codes(packed, n)
    wk = lettermodel.walk(letter, codes, tasks, 5)
    assert (wk.w == w).all(), (name, letter, int(np.flatnonzero(wk.w != w)[0]))
    # what the product hands on after a letter's block is what its tasks start from, whatever it was handed
    assert end == lettermodel.MAIN_START[letter]
    # the start state changes no w, and the letter-free inputs are those of 'B'
    packed_b, n_b, tasks_b, w_b, _ = hip.host_wavelet_elements(args, 0)
    assert n_b == n and (packed_b == packed).all() and (tasks_b == tasks).all()
    _, _, _, w0, _ = hip.host_wavelet_elements(args, 0, letter=letter)
    assert (w0 == w).all()
    if name != "all_equal" or (tasks[:, 2] == ROOT).any():
        assert (w_b != w).any(), (name, letter)
    # ... and the host lanes on the real elements
    wl, endl = hip.host_test_models(packed, n, tasks, 2, letter=letter)
    assert (wl == wk.w).all() and endl == lettermodel.MAIN_START[letter], (name, letter)


@pytest.mark.parametrize("letter", LETTERS)
@pytest.mark.parametrize("name", lettermodel.CASE_NAMES)
def test_host_lanes_match_the_walk(name, letter):
    from bwtc_amd import hip
    c = lettermodel.case(name)
    wk = lettermodel.case_walk(letter, name)
    w, end = hip.host_test_models(c.packed, c.n, c.tasks, c.state_in, letter=letter)
    assert (w == wk.w).all(), (name, letter, int(np.flatnonzero(w != wk.w)[0]))
    assert end == lettermodel.MAIN_START[letter]
    w7, _ = hip.host_test_models(c.packed, c.n, c.tasks, 7 - c.state_in, letter=letter)
    assert (w7 == w).all(), (name, letter)


@pytest.mark.parametrize("letter", LETTERS)
@pytest.mark.parametrize("name", lettermodel.CASE_NAMES)
def test_case_tells_the_letter_from_B(name, letter):
    """A route that quietly ran the 'B' models would not give the walk's w on any case."""
    c = lettermodel.case(name)
    assert c.n <= 400000
    assert (gmmodel.walk(c.codes, c.tasks, c.state_in).w != lettermodel.case_walk(letter, name).w).any(), (name, letter)


def test_walk_does_not_look_at_the_carried_state():
    c = lettermodel.case("tiny_ladder")
    for letter in LETTERS:
        a, b = lettermodel.walk(letter, c.codes, c.tasks, 0), lettermodel.walk(letter, c.codes, c.tasks, 7)
        assert (a.w == b.w).all() and (a.states == b.states).all() and (a.state_out, b.state_out) == (0, 7)


# ---- every named case is what its name says ----------------------------------------------------------------

def _chunks(c):
    ch, _ = gmmodel.cut_chunks(c.tasks)
    return ch.astype(np.int64)


@pytest.mark.parametrize("name", lettermodel.SINGLE_CASES)
def test_single_cases(name):
    c = lettermodel.case(name)
    _, ty, n = name.split("_")
    assert c.tasks.tolist()[0] == [0, int(n), {v: k for k, v in lettermodel.TYPE_NAMES.items()}[ty]]
    assert int(n) in lettermodel.SINGLE_LENGTHS and c.tasks.shape[0] == 2 and c.n == int(n) + 5
    own = [int(e - b) for b, e, tf in _chunks(c) if tf & 0x7FFFFFFF == 0]
    assert own == [CHUNK] * (int(n) // CHUNK) + ([int(n) % CHUNK] if int(n) % CHUNK else [])


def test_tasks_meet_at_every_offset_around_a_grid_line():
    c = lettermodel.case("meet_grid")
    t = c.tasks.astype(np.int64)
    starts = t[1:, 0]
    assert sorted(set(((starts + 64) % CHUNK).tolist()) & set(range(128))) == list(range(128))
    for letter in LETTERS:
        wk = lettermodel.case_walk(letter, "meet_grid")
        # every task starts from the start state ...
        assert (wk.states[t[:, 0]] == (lettermodel.MAIN_START[letter] | 2 << 3 | 1 << 5)).all()
    # ... and under 'b' the element before most starts has left the main machine elsewhere: a reset that only reached
    # gaps and integers would show
    wk = lettermodel.case_walk("b", "meet_grid")
    prev_ty = t[:-1, 2]
    moved = [(int(wk.states[s - 1]) & 7) for s, ty in zip(starts.tolist(), prev_ty.tolist()) if ty in (ROOT, INNER)]
    assert len(moved) >= 60 and len(set(moved)) >= 5
    # the state scan's places: a task start as a thread's first and last chunk of eight, and inside
    first = _chunks(c)[:, 2] >> 31
    places = set((np.flatnonzero(first) % 8).tolist())
    assert {0, 7} <= places and places - {0, 7}, places


@pytest.mark.parametrize("name,ty", [("tails_root", ROOT), ("tails_inner", INNER)])
def test_tail_cases(name, ty):
    """Chunks that end at a grid line with their task going on: the last flip is the chunk's last, last-but-one or
    last-but-two advancing element (every element of these tasks advances the machine), or lies further back / nowhere;
    chunks of one and two elements take the full walk."""
    c = lettermodel.case(name)
    ch = _chunks(c)
    bits = (c.codes & 1).astype(np.int64)
    seen, short = set(), set()
    for i in range(len(ch) - 1):
        b, e, tf = ch[i]
        if c.tasks[tf & 0x7FFFFFFF, 2] != ty or e % CHUNK or (ch[i + 1, 2] >> 31):
            continue
        x = bits[b:e][::-1]
        flips = np.flatnonzero(x[1:] != x[:-1])
        run = int(flips[0]) + 1 if flips.size else None          # equal bits at the end; None: the whole chunk
        if e - b < 3:
            short.add((int(e - b), run))
        elif e - b <= 100:
            seen.add((min(run, 4) if run else 4, int(x[0])))
    assert seen >= {(r, v) for r in (1, 2, 3, 4) for v in (0, 1)}, seen
    assert {k for k, _ in short} == {1, 2} and (2, 1) in short and (2, None) in short, short
    # under 'b' the states after such chunks take every value the rule can give
    wk = lettermodel.case_walk("b", name)
    after = {int(wk.states[e]) & 7 for b, e, tf in ch[:-1] if e % CHUNK == 0 and e < c.n}
    assert after == set(range(6)), after


def test_inner_gap_flags_fall_between_the_main_machines_steps():
    c = lettermodel.case("inner_gaps")
    wk = lettermodel.case_walk("b", "inner_gaps")
    flag = (c.codes >> 1).astype(bool)
    assert (c.tasks[:, 2] == INNER).all() and 1000 < flag.sum() < c.n - 1000
    assert (wk.slot[flag] >= 8).all() and (wk.slot[~flag] < 6).all()
    # the machine moves under a flagged element (the state before the next element differs) and its predictor does not
    inside = np.flatnonzero(flag[:-1] & ~np.isin(np.arange(c.n - 1) + 1, c.tasks[:, 0]))
    assert np.count_nonzero((wk.states[inside] & 7) != (wk.states[inside + 1] & 7)) > 500
    for i in inside[:2000].tolist():
        k = int(wk.states[i]) & 7                                  # the main slot a flagged element would have named
        later = np.flatnonzero((wk.slot[i + 1:i + 200] == k))
        same_task = [t for t in c.tasks.tolist() if t[0] <= i < t[1]][0]
        if later.size and i + 1 + int(later[0]) < same_task[1]:
            j = i + 1 + int(later[0])
            earlier = np.flatnonzero(wk.slot[same_task[0]:i] == k)
            want = 2048 if not earlier.size else lettermodel.counter(int(wk.before[same_task[0] + earlier[-1]]),
                                                                     int(c.codes[same_task[0] + earlier[-1]]) & 1)
            assert wk.before[j] == want, (i, j)
    # chunks of these tasks end at grid lines too
    assert any(e % CHUNK == 0 for _, e, _ in _chunks(c)[:-1])


def _alive(stream, j):
    """Distinct end values of the three start values over slot-chunk j of a chain that starts at position 0."""
    return len(set(lettermodel.images(stream[j * SLOT_CHUNK:(j + 1) * SLOT_CHUNK])))


@pytest.mark.parametrize("name", lettermodel.ALT_CASES)
def test_alternating_cases_keep_two_values_alive(name):
    """'u', one root task: slot space is the task itself.  Over every whole slot-chunk of alternating bits two of the
    three start values stay apart, and so they do over a whole chain group of sixteen slot-chunks; a doubled bit merges
    them within its own slot-chunk only."""
    c = lettermodel.case(name)
    wk = lettermodel.case_walk("u", name)
    assert c.tasks.tolist() == [[0, 40000, ROOT]] and (wk.slot == 0).all()
    stream = lettermodel.slot_stream(c, wk, 0)
    nsc = (c.n + SLOT_CHUNK - 1) // SLOT_CHUNK
    assert nsc == 20 and nsc > 16
    same = np.flatnonzero(stream[1:] == stream[:-1]) + 1
    if name.startswith("alt_from"):
        assert same.size == 0 and int(stream[0]) == int(name[-1])
        assert all(_alive(stream, j) == 2 for j in range(nsc))
        assert len(set(lettermodel.images(stream[:16 * SLOT_CHUNK]))) == 2          # across the chain-group border
        assert len(set(lettermodel.images(stream[SLOT_CHUNK:19 * SLOT_CHUNK]))) == 2
    else:
        at = lettermodel.DOUBLED_BORDER + {"before": -1, "at": 0, "after": 1}[name.split("_")[-1]]
        assert same.tolist() == [at]
        # the slot-chunk that holds both bits of the pair has a constant map; where the pair lies across the border every
        # slot-chunk keeps two values apart and the two maps around the border merge them
        jd = at // SLOT_CHUNK if at % SLOT_CHUNK else -1
        assert [_alive(stream, j) for j in range(nsc)] == [1 if j == jd else 2 for j in range(nsc)]
        b = lettermodel.DOUBLED_BORDER
        assert len(set(lettermodel.images(stream[b - SLOT_CHUNK:b + SLOT_CHUNK]))) == 1


def test_period6_makes_the_stream_of_state_3_alternate():
    c = lettermodel.case("period6")
    wk = lettermodel.case_walk("b", "period6")
    assert c.n == 3 * 6 * SLOT_CHUNK + 5 and c.tasks.shape[0] == 1
    s3 = lettermodel.slot_stream(c, wk, 3)
    assert s3.size >= 3 * SLOT_CHUNK and (s3[1:] != s3[:-1]).all()
    assert (wk.w != lettermodel.case_walk("u", "period6").w).any()                  # the two letters differ here
    # its chain lies behind those of states 0 ... 2 in slot space and crosses slot-chunk borders with two values alive
    p0 = int(np.count_nonzero(wk.slot < 3))
    first = -(-p0 // SLOT_CHUNK)
    borders = [j * SLOT_CHUNK - p0 for j in range(first + 1, (p0 + s3.size) // SLOT_CHUNK + 1)]
    assert len(borders) >= 2
    for a, z in zip(borders[:-1], borders[1:]):
        assert len(set(lettermodel.images(s3[a:z]))) == 2


@pytest.mark.parametrize("name,bit", [("all_zeros", 0), ("all_ones", 1)])
def test_constant_cases_saturate(name, bit):
    c = lettermodel.case(name)
    assert ((c.codes & 1) == bit).all()
    for letter in LETTERS:
        wk = lettermodel.case_walk(letter, name)
        main = wk.slot < 8
        # a main slot stands at its bound after two elements: every later element is coded with the same probability
        sat = 3072 if bit else 1024
        assert np.count_nonzero(wk.before[main] != sat) <= 2 * 6 * c.tasks.shape[0]
        assert np.count_nonzero(wk.before[main] == sat) > 3 * SLOT_CHUNK
        for j in range(1, 3):
            assert lettermodel.images(np.full(SLOT_CHUNK, bit)) == [sat] * 3
