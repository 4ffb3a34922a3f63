"""CPU tests of tests/prblocks.py: every builder's premise proved with the oracle alone (oracle_pair_statistics,
oracle_pair_replace_round, the grammar it leaves), so that no test of tests/test_gpu_prepr_limits.py can pass on a block
that does not do what its name says; and the numpy restatement of the counting rule against the oracle's counters."""
import numpy as np
import pytest

import prblocks as pb

REPLACES = 2100                                               # from here on pairs_on_seams has a pair above 1003


def _round(oracle, data):
    g = oracle.OracleGrammar()
    rep, w = oracle.oracle_pair_replace_round(g, data)
    return rep, w, g.write()


def _same_counts(oracle, data, what):
    f, pf = oracle.oracle_pair_statistics(data)
    bf, bp = pb.pair_counts(data)
    assert (f == bf).all(), what
    assert (pf == bp).all(), (what, np.flatnonzero(pf != bp)[:4])
    assert int(pf.sum()) <= data.size - 1 and int(f.sum()) == data.size


def test_sizes_sit_on_the_kernels_grains():
    s = pb.sizes()
    assert s == sorted(set(s)) and s[0] == 3
    for k in (1, 2, 512, 1024):
        assert {k * pb.TILE - 1, k * pb.TILE + 1} & set(s), k
    assert {15, 16, 17, 4096 + 15, 4096 + 16, 4096 + 17} <= set(s)
    assert max(s) > 1024 * pb.TILE + pb.TILE and max(s) < 1 << 23


@pytest.mark.parametrize("n", pb.sizes())
def test_counting_rule_restated_matches_the_oracle(oracle, n):
    for name, data in pb.stat_edges(n, 1).items():
        assert data.size == n and data.dtype == np.uint8
        _same_counts(oracle, data, (name, n))
    for ending in pb.ENDINGS:
        _same_counts(oracle, pb.pairs_on_seams(n, ending), (ending, n))
    if n <= pb.SMALL:
        for where in pb.WHERE:
            _same_counts(oracle, pb.double_runs(n, where), (where, n))


def test_counting_rule_restated_on_the_other_builders(oracle):
    for name, data in (("long", pb.long_double_run()), ("tile1024", pb.run_at_tile_1024()),
                       ("decides", pb.one_count_decides(1004)), ("decides_double", pb.one_count_decides_double(1003)),
                       ("escaped", pb.all_escaped_tile()), ("rounds", pb.rounds_to_exhaustion(1))):
        _same_counts(oracle, data, name)


@pytest.mark.parametrize("n", [4096 + 18, 8193])
def test_stat_edges_hold_what_they_name(n):
    e = pb.stat_edges(n, 1)
    assert set(np.unique(e["sigma2"])) == {0, 0xC1} and np.unique(e["sigma3"]).size == 3
    assert not e["zeros"].any() and (e["ff"] == 0xFF).all()
    assert not e["start000"][:3].any() and e["start000"].any()
    q = e["quarters"]
    seen = set(zip(q[:-1].tolist(), q[1:].tolist()))
    assert seen == {(a, b) for a in pb.QUARTERS for b in pb.QUARTERS}          # every edge as first and as second byte
    for name in ("sigma2", "sigma3"):                         # three equal bytes ending at odd and at even positions
        d = e[name]
        ends = np.flatnonzero((d[2:] == d[1:-1]) & (d[1:-1] == d[:-2])) + 2
        assert (ends & 1).any() and not (ends & 1).all()
        assert {int(v) % 16 for v in ends} == set(range(16))
    for d in pb.TRIPLE_AT:
        t = e["triples%+d" % d]
        starts = pb.triple_starts(n, d)
        assert {s - d for s in starts} >= set(range(16, n - 4, 16)) and pb.TILE + d in starts
        for s in starts:
            assert t[s] == t[s + 1] == t[s + 2] and t[s - 1] != t[s] and (s + 3 == n or t[s + 3] != t[s])


@pytest.mark.parametrize("ending", pb.ENDINGS)
@pytest.mark.parametrize("n", pb.sizes())
def test_pairs_on_seams_premise(oracle, n, ending):
    data = pb.pairs_on_seams(n, ending)
    assert data.size == n
    rep, w, raw = _round(oracle, data)
    if n < REPLACES:
        assert rep == 0 and w.tobytes() == data.tobytes()
        return
    _, pf = oracle.oracle_pair_statistics(data)
    assert pf[pb.A << 8 | pb.B] > 1003 + 3
    assert rep >= 1 and bytes([pb.A, pb.B]) in pb.replaced_pairs(raw)
    start, in_len, out_len = pb.tokens(raw, w)
    assert int(in_len.sum()) == n
    seams = set(range(16, pb.seam_limit(n, ending) + 1, 16))
    assert seams and seams <= pb.straddled(raw, w)
    assert all(s in seams for s in range(pb.TILE, n - 5, pb.TILE))
    if ending == "pair":
        assert start[-1] == n - 2 and in_len[-1] == 2 and out_len[-1] == 1
    elif ending == "first":
        assert start[-1] == n - 1 and in_len[-1] == 1 and out_len[-1] == 1 and data[n - 1] == pb.A
        assert start[-2] == n - 3 and in_len[-2] == 2
    else:
        assert start[-1] == n - 1 and in_len[-1] == 1 and out_len[-1] == 2      # the last byte is written as an escape
        assert start[-2] == n - 3 and in_len[-2] == 2
        assert (out_len == 2).sum() == 1 + 2 + 3                                  # the three rarest symbols, nothing else


def _runs_of_x(data):
    x = np.concatenate([[False], data == pb.X, [False]])
    edge = np.flatnonzero(x[1:] != x[:-1])
    return edge[0::2], edge[1::2]                              # first positions, positions behind the last


@pytest.mark.parametrize("where", pb.WHERE)
@pytest.mark.parametrize("n", [4094, 4096 + 18, 8193, 512 * 4096 + 1])
def test_double_runs_premise(oracle, n, where):
    data = pb.double_runs(n, where)
    assert data.size == n
    rep, w, raw = _round(oracle, data)
    assert rep >= 1 and bytes([pb.X, pb.X]) in pb.replaced_pairs(raw)
    a, b = _runs_of_x(data)
    inner = (a > 0) & (b < n)
    a, b = a[inner], b[inner]
    assert {int(v) % 16 for v in a} == {15, 0, 1} and {int(v) % 16 for v in b} == {15, 0, 1}
    combos = {(int(s) % 16, int(e) % 16, int(e - s) & 1) for s, e in zip(a, b)}
    assert len({c[:2] for c in combos}) == 9 and {c[2] for c in combos} == {0, 1}
    # what happens at the tile seam
    seam = pb.TILE
    if n < seam + 64:
        pass
    elif where == "through":
        assert ((a < seam - 16) & (b > seam + 16)).any()
    else:
        at = seam + int(where[-2:])
        assert at in (a if where.startswith("start") else b).tolist()
    # the oracle pairs every run from its start: its tokens say so
    start, in_len, _ = pb.tokens(raw, w)
    pair_starts = set(start[in_len == 2].tolist())
    for s, e in list(zip(a.tolist(), b.tolist()))[:200]:
        assert all(p in pair_starts for p in range(s, e - 1, 2)), (s, e)


def test_long_double_run_premise(oracle):
    data = pb.long_double_run()
    a, b = _runs_of_x(data)
    k = int(np.argmax(b - a))
    assert a[k] == pb.LONG_RUN_START and a[k] & 1 and b[k] - a[k] == pb.LONG_RUN == 1024 * 4096 + 4096 + 3
    assert a[k] < pb.TILE and b[k] > 1025 * pb.TILE          # from tile 0 into the head scan's second chunk
    assert b.size > k + 3 and data.size < 1 << 23
    rep, w, raw = _round(oracle, data)
    assert rep >= 1 and bytes([pb.X, pb.X]) in pb.replaced_pairs(raw)


def test_run_at_tile_1024_premise(oracle):
    data = pb.run_at_tile_1024()
    assert data.size == 1025 * pb.TILE + 17
    a, b = _runs_of_x(data)
    assert 1024 * pb.TILE in a.tolist() and data[1024 * pb.TILE - 1] != pb.X
    assert b[a.tolist().index(1024 * pb.TILE)] == data.size - 30
    rep, w, raw = _round(oracle, data)
    assert rep >= 1 and bytes([pb.X, pb.X]) in pb.replaced_pairs(raw)


@pytest.mark.parametrize("double", [False, True])
def test_one_count_decides_premise(oracle, double):
    build = pb.one_count_decides_double if double else pb.one_count_decides
    pair = (pb.X, pb.X) if double else pb.P
    for k in (1003, 1004):
        data = build(k)
        assert data.size == pb.DECIDE_TILES * pb.TILE
        f, pf = oracle.oracle_pair_statistics(data)
        assert (f == 0).sum() >= 2                             # unused symbols: a variable costs nothing
        assert pf[pair[0] << 8 | pair[1]] == k
        others = pf.copy()
        others[pair[0] << 8 | pair[1]] = 0
        assert others.max() < 100
        at = np.flatnonzero((data[:-1] == pair[0]) & (data[1:] == pair[1]))
        if double:
            a, b = _runs_of_x(data)
            assert ((b - a) == 3).all()
            assert {int(v) % 16 for v in a} == {14, 15}       # triples start two and one before a seam
            assert set(range(pb.TILE, data.size, pb.TILE)) <= set((a + 1).tolist()) | set((a + 2).tolist())
            assert (a & 1).sum() + 2 * ((a & 1) == 0).sum() == k
        else:
            assert at.size == k and ((at + 1) % 16 == 0).all()
            assert set(range(pb.TILE, data.size, pb.TILE)) <= set((at + 1).tolist())
        rep, w, raw = _round(oracle, data)
        assert rep == (1 if k == 1004 else 0)
        assert (bytes(pair) in pb.replaced_pairs(raw)) == (k == 1004)


def test_all_escaped_tile_premise(oracle):
    data = pb.all_escaped_tile()
    f, pf = oracle.oracle_pair_statistics(data)
    assert (f > 0).all()
    assert sorted(np.argsort(f, kind="stable")[:4].tolist()) == list(pb.RAREST) and np.sort(f)[4] > f[1] == 1024
    assert set(np.unique(data[:pb.TILE]).tolist()) == set(pb.RAREST) and not np.isin(data[pb.TILE:], pb.RAREST).any()
    for a in pb.RAREST:
        for b in pb.RAREST:
            assert pf[a << 8 | b] < 1004
    g = oracle.OracleGrammar()
    rep, w = oracle.oracle_pair_replace_round(g, data)
    assert rep == 2 and g.specials == 2
    assert pb.replaced_pairs(g.write()) == {bytes(p) for p in pb.FREQUENT}
    special = np.array([g.is_special(c) for c in range(256)])
    assert special[w[:2 * pb.TILE]].all() and not special[w[2 * pb.TILE]]
    start, in_len, out_len = pb.tokens(g.write(), w)
    assert (out_len[:pb.TILE] == 2).all() and start[pb.TILE] == pb.TILE


def test_rounds_to_exhaustion_premise(oracle):
    data = pb.rounds_to_exhaustion(1)
    assert data.size == 1 << 20
    g = oracle.OracleGrammar()
    productive = 0
    for _ in range(pb.ROUNDS_CAP):
        rep, w = oracle.oracle_pair_replace_round(g, data)
        if rep == 0:
            assert w.tobytes() == data.tobytes()
            break
        assert w.size < data.size
        productive += 1
        data = w
    else:
        pytest.fail("the rounds do not end within %d" % pb.ROUNDS_CAP)
    assert productive >= 7 and g.specials >= 2
