"""CPU tests of tests/gmmodel.py -- the sequential model the GPU model passes are held to in
tests/test_gpu_model_passes.py -- and of the passes themselves run lane by lane on the host.

The anchor: the model's w equals the w of the product's SEQUENTIAL host coder (StreamCoder::model over
planStreams / expandStreamsOnHost, bwtc_hip_host_wavelet_elements) on real blocks, from all eight start states
and with the state carried over two blocks; that coder's bytes are held equal to the oracle's in
tests/test_host_logic.py.  Then: every hand-built case reaches the edges it was built for (measured from the
model alone), the host lanes (bwtc_hip_host_test_models) give the model's w and end state on every case, and
the derived expectations agree with the plain walk on random small inputs.

Of the limit blocks of tests/blockgen.py, fib_depth has 24 million one-byte runs and far more coded elements
than a Python loop can walk (the model's cases stay below 400 000): sections_inside_runs and many_ids are used."""
import numpy as np
import pytest

import blockgen
import gmmodel
from test_host_logic import _runs_of


def _section_args(bwt, sections):
    """The section-run arguments of bwtc_hip_host_wavelet_streams for a transformed block."""
    first, syms, starts, rfs, doff, dl, dc, beg = [0], [], [], [], [0], [], [], 0
    for n in sections:
        sy, st = _runs_of(bwt[beg:beg + int(n)])
        syms.append(sy)
        starts.append(st[:-1] + np.uint32(beg))
        first.append(first[-1] + sy.size)
        rfs.append(np.bincount(sy, minlength=256).astype(np.uint32))
        u, c = np.unique(np.diff(st.astype(np.int64)), return_counts=True)
        dl.append(u.astype(np.uint32))
        dc.append(c.astype(np.uint32))
        doff.append(doff[-1] + u.size)
        beg += int(n)
    return (len(sections), np.array(first, np.uint32), np.concatenate(syms).astype(np.uint8),
            np.concatenate(starts + [np.array([beg], np.uint32)]).astype(np.uint32), np.concatenate(rfs),
            np.array(doff, np.uint32), np.concatenate(dl), np.concatenate(dc))


def _anchor_blocks(oracle):
    from bwtc_amd import synth
    rng = np.random.default_rng(31)
    blocks = []
    kinds = set()
    while len(kinds) < 7:                                 # every kind of blockgen.structured once
        kind, d = blockgen.structured(rng, int(rng.integers(1500, 4000)))
        if kind not in kinds:
            kinds.add(kind)
            blocks.append(("structured_%d" % kind, d, True))
    blocks.append(("text", synth.gen_text(12000, 5), True))
    for name, block, _ in blockgen.limit_blocks(names=("sections_inside_runs", "many_ids")):
        blocks.append((name, block, False))               # used as transformed blocks, as the limit tests do
    out = []
    for name, d, transform in blocks:
        if transform:
            bwt, _, freqs = oracle.oracle_bwt_block(d, 4)
        else:
            bwt, freqs = d, np.bincount(d, minlength=256).astype(np.uint32)
        out.append((name, _section_args(bwt, oracle.oracle_sections(freqs))))
    return out


def test_model_matches_the_sequential_host_coder(oracle):
    from bwtc_amd import hip
    blocks = _anchor_blocks(oracle)
    elements = {}
    for name, args in blocks:
        for state in range(8):
            packed, n, tasks, w, end = hip.host_wavelet_elements(args, state)
            assert 0 < n <= 400000, (name, n)
            codes = gmmodel.unpack_codes(packed, n)
            assert (gmmodel.pack_codes(codes) == packed).all()
            wk = gmmodel.walk(codes, tasks, state)
            assert (wk.w == w).all(), (name, state, int(np.flatnonzero(wk.w != w)[0]))
            assert wk.state_out == end, (name, state)
            assert gmmodel.end_states(codes, tasks)[state] == end, (name, state)
            elements[name] = (codes, tasks)
    # the state carried over two consecutive blocks
    for (a, args_a), (b, args_b) in zip(blocks[:-1], blocks[1:]):
        for state in (0, 3, 7):
            _, _, _, _, mid = hip.host_wavelet_elements(args_a, state)
            _, _, _, w, end = hip.host_wavelet_elements(args_b, mid)
            mid_model = gmmodel.walk(*elements[a], state).state_out
            wk = gmmodel.walk(*elements[b], mid_model)
            assert mid_model == mid and (wk.w == w).all() and wk.state_out == end, (a, b, state)


@pytest.mark.parametrize("name", gmmodel.CASE_NAMES)
def test_case_reaches_its_edges(name):
    """Every hand-built case reaches the measures of its `edge` (gmmodel.measures: from the model alone), stays
    within the size a Python reference can walk, and is valid input for the hooks."""
    c = gmmodel.case(name)
    assert c.n <= 400000
    t = c.tasks.astype(np.int64)
    assert t[0, 0] == 0 and t[-1, 1] == c.n and (t[1:, 0] == t[:-1, 1]).all() and (t[:, 1] > t[:, 0]).all() and (t[:, 2] <= 3).all()
    assert (gmmodel.unpack_codes(c.packed, c.n) == c.codes).all()
    assert gmmodel.edge_misses(c) == {}, name


def test_open_brackets_strictly_inside_by_slot_kind():
    """A true start value strictly inside an open bracket, for each (floor, delay) pair.  Integer slots reach it with
    periodic element patterns (period 6 and 8).  For the main and gap slots no periodic element pattern does; a search
    over the bits of one chain (prefix of up to 8 bits, then a period of up to 8) found chains that do, and the case
    feeds them to slot 11 and slot 7 through the elements between (gmmodel._gaps_for_slot11, _root_for_slot7).
    Also: the widest bracket, 2^d - 1, with the true value on its lowest and on its highest candidate."""
    m = gmmodel.measures(gmmodel.case("open_brackets"))
    print("open_brackets: (floor 2, delay 4)", sorted(m["bracket_2_4"]), "(2, 5)", sorted(m["bracket_2_5"]),
          "(100, 5)", sorted(m["bracket_100_5"]), "inside:", m["inside_2_4"], m["inside_2_5"], m["inside_100_5"])
    assert m["inside_100_5"] >= 1 and m["inside_2_5"] >= 1 and m["inside_2_4"] >= 1
    assert {(15, "low"), (15, "top")} <= m["bracket_2_4"]
    assert {(31, "low"), (31, "top")} <= m["bracket_2_5"] and {(31, "low"), (31, "top")} <= m["bracket_100_5"]


@pytest.mark.parametrize("name", gmmodel.CASE_NAMES)
def test_host_lanes_match_the_model(name):
    """The passes lane by lane on the host, in buffers of exactly the device's sizes: the model's w and end state."""
    from bwtc_amd import hip
    c = gmmodel.case(name)
    states = range(8) if name in gmmodel.SCAN_CASES and c.n < 20000 else (c.state_in,)
    for s in states:
        wk = c.walk(s)
        w, end = hip.host_test_models(c.packed, c.n, c.tasks, s)
        assert (w == wk.w).all(), (name, s, int(np.flatnonzero(w != wk.w)[0]))
        assert end == wk.state_out, (name, s)


def test_host_hook_refuses_invalid_input():
    from bwtc_amd import hip
    c = gmmodel.case("tiny_ladder")
    for packed, n, tasks, state in _invalid_inputs(c):
        with pytest.raises(hip.BwtcHipError) as e:
            hip.host_test_models(packed, n, tasks, state)
        assert e.value.code == -1


def _invalid_inputs(c):
    """(packed, n_coded, tasks, state_in) that the hooks refuse: a type above 3, an empty task, a hole, an overlap,
    tasks out of order, tasks that stop short of n_coded or go past it, and a state above 7."""
    t = c.tasks.copy()
    bad = []
    for change in ("type", "empty", "hole", "overlap", "order", "short", "long"):
        x = t.copy()
        if change == "type":
            x[3, 2] = 4
        elif change == "empty":
            x[5, 1] = x[5, 0]
        elif change == "hole":
            x[7, 0] += 1
        elif change == "overlap":
            x[7, 0] -= 1
        elif change == "order":
            x[[2, 3]] = x[[3, 2]]
        elif change == "short":
            x = x[:-1]
        else:
            x[-1, 1] += 1
        bad.append((c.packed, c.n, x, c.state_in))
    bad.append((c.packed, c.n, t, 8))
    return bad


def test_derived_expectations_agree_with_the_plain_walk():
    """On random small inputs: the gather, un-gathered, gives back the bits; the value at a slot-space position is the
    walk's value before that element; chains are contiguous and start from the slot's initial value; base and sb count
    every element once; the state at a chunk's start, walked over the chunk, is the state at the next chunk's start."""
    rng = np.random.default_rng(8)
    for it in range(40):
        b = gmmodel._Builder(1000 + it)
        for _ in range(int(rng.integers(1, 30))):
            b.runs(int(rng.integers(0, 4)), int(rng.integers(1, 900)), mean=int(rng.choice([2, 20])))
        c = b.case("random", int(rng.integers(0, 8)), {})
        wk, ex = c.walk(), c.expect()
        n, nc, nt = c.n, ex.nc, ex.nt
        # the gather is a permutation; un-gathered it gives the bits back
        assert (np.sort(ex.order) == np.arange(n)).all()
        back = np.zeros(n, np.uint8)
        back[ex.order] = (ex.sbits[:, None] >> np.arange(32, dtype=np.uint32) & 1).reshape(-1)[:n]
        assert (back == (c.codes & 1)).all()
        assert (ex.sbits.reshape(-1)[(n + 31) // 32:] == 0).all() and ex.sbits.size == n // 32 + 16
        # slot-major, then task, then order
        task_of = np.repeat(np.arange(nt), (c.tasks[:, 1] - c.tasks[:, 0]).astype(np.int64))
        key = wk.slot[ex.order] * (nt * (n + 1)) + task_of[ex.order] * (n + 1) + ex.order
        assert (np.diff(key) > 0).all()
        # stream starts: every (slot, task) stream is where its elements are
        sb = ex.sb.astype(np.int64)
        assert sb[0] == 0 and sb[-1] == n and (np.diff(sb) >= 0).all()
        for k in range(gmmodel.SLOTS):
            for t in range(nt):
                a, z = sb[k * nt + t], sb[k * nt + t + 1]
                assert (wk.slot[ex.order[a:z]] == k).all() and (task_of[ex.order[a:z]] == t).all()
                if z > a:
                    assert ex.val[a] == gmmodel.slot_init(k)
                    assert (ex.val[a + 1:z] == ex.val_after[a:z - 1]).all()          # a chain: each value follows from the one before
        assert (ex.val == wk.before[ex.order]).all()
        assert int(ex.base[-1]) == n and int(ex.base[15 * nc]) == n
        # chunk states
        ch = ex.chunks.astype(np.int64)
        for i in range(nc):
            t = int(ch[i, 2] & 0x7FFFFFFF)
            m8, m4, m3 = gmmodel.machines_over(c.codes, int(ch[i, 0]), int(ch[i, 1]), int(c.tasks[t, 2]))
            s = int(ex.cstate[i])
            after = m8[s & 7] | m4[(s >> 3) & 3] << 3 | m3[(s >> 5) & 3] << 5
            if i + 1 < nc:
                nxt = int(ex.cstate[i + 1])
                if ch[i + 1, 2] >> 31:
                    assert nxt == (after & 7) | 2 << 3 | 1 << 5
                else:
                    assert nxt == after
            else:
                assert after & 7 == wk.state_out
        # the honest bracket holds the true value, and its candidates' images hold the true end value
        for j in range(1, ex.nsc):
            L, width = ex.bracket(j)
            assert L <= ex.val[j * gmmodel.SLOT_CHUNK] <= L + width
            if width and ex.starts_inside(j) == 0:
                img = ex.candidate_images(j)
                p1 = min((j + 1) * gmmodel.SLOT_CHUNK, n)
                assert img[int(ex.val[j * gmmodel.SLOT_CHUNK]) - L] == ex.val_after[p1 - 1]
                assert (np.diff(img) >= 0).all() and (np.diff(img) <= 1).all()
