"""The finder's candidates under BWTC_HIP_MULTI on the GPU (-m gpu), through the hook bwtc_hip_test_period_winners:
k_period_winners, one workgroup over the table of 4097 vote bins in the context's own buffer, held to
tests/multimodel.py's candidates() -- up to 8 (distance, votes) pairs with a distance in 2 ... 4096 and `need` votes or
more, by descending votes, the smaller distance first among equals -- and the 16 words it leaves to zeros behind them.
The tables are tests/multicases.py's; tests/test_multimodel.py states what each must give.

Without the feature the hook does not exist."""
import numpy as np
import pytest

import multicases as cases
import multimodel as mu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from bwtc_amd import hip
    c = hip.Context(0, 1 << 20)
    yield c
    c.close()


def _same(ctx, table, need, what):
    want = mu.candidates(table, need)
    got, words = ctx.test_period_winners(table, need)
    assert got == want, (what, need, got, want)
    flat = [x for pair in want for x in pair]
    assert words.tolist() == flat + [0] * (16 - len(flat)), (what, need, words.tolist())
    return got


@pytest.mark.parametrize("need", [256, (1 << 20) // 64])
def test_the_named_tables(ctx, need):
    """No bin over need, one, exactly 8 and more than 8, equal votes, bins 2 and 4096, votes planted in bins 0 and 1, every
    bin at need, votes of 32 bits; need of 256 and of n / 64."""
    seen = {name: _same(ctx, table, need, name) for name, table in cases.vote_tables(need)}
    assert seen["no bin over need"] == [] and len(seen["more than 8"]) == 8
    assert [d for d, _ in seen["equal votes"]] == [2, 5, 6, 17, 18, 250, 999, 1000]
    assert seen["votes in bins 0 and 1"] == [(33, need)]


def test_random_tables_and_a_block_s_own(ctx):
    rng = np.random.default_rng(59)
    for it in range(40):
        table = rng.integers(0, 1000, 4097).astype(np.uint32)
        if it % 2:
            table[rng.integers(0, 4097, 30)] = rng.integers(900, 1100, 30)
        _same(ctx, table, int(rng.integers(1, 1100)), it)
    _same(ctx, np.zeros(4097, np.uint32), 0, "an empty table and need 0")
    T = cases.stretches((9, 12), 1 << 15)
    got = _same(ctx, cases.vote_table(T, 8), max(256, T.size // 64), "a block's table")
    assert {9, 12} <= {d for d, _ in got}
