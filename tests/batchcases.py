"""Named batches for the batched transform's tests (tests/batchmodel.py states the rule): every case says which seam
or limit it sits on, and `premise` proves it from the blocks and the model's result, so that a case cannot quietly
stop exercising what it is named for.  Shared by tests/test_batchmodel.py (no GPU) and tests/test_gpu_batch_bwt.py;
models and oracle results are computed once per process."""
import functools

import numpy as np

import batchmodel

LOAD_TILE = 4096          # positions a workgroup of k_batch_load takes
LOAD_PER_THREAD = 16      # ... and a thread of it
LDS_HIST_FROM = 256       # strides from which a block counts in an LDS histogram


def _rng(seed):
    return np.random.default_rng(seed)


def _rand(rng, size, sigma=256):
    return rng.integers(0, sigma, size, dtype=np.uint8)


def _text(size, seed):
    from bwtc_amd import synth
    return np.ascontiguousarray(synth.gen_text(size, seed)[:size])


def _period2(size, a=0x61, b=0x62):
    out = np.empty(size, np.uint8)
    out[0::2], out[1::2] = a, b
    return out


# ---- the cases: name -> (blocks, starting points) -----------------------------------------------------------------
def _same(count):
    def make():
        blk = _rand(_rng(11), 700, 3)
        return [blk.copy() for _ in range(count)], 8
    return make


def _seam_end_begin():
    # sizes 2^k - 1: n_b = S, no padding between T_b and T_(b+1); every block ends as the next one begins, and the
    # blocks are deep (two letters, long repeats): a look-up that crossed the seam would find a rank where the rule says 0
    rng = _rng(12)
    a = _period2(1023)
    b = np.concatenate([a[-400:], np.zeros(300, np.uint8), _rand(rng, 323, 2)])
    c = np.concatenate([b[-400:], _period2(623)])
    z = np.zeros(1023, np.uint8)
    return [a, b, c, z, z, np.concatenate([z[:500], _rand(rng, 523, 2)])], 8


def _seam_reverse():
    rng = _rng(13)
    a = _rand(rng, 1023, 2)
    b = np.concatenate([_period2(600), _rand(rng, 423, 2)])
    return [a, a[::-1].copy(), b, b[::-1].copy()], 8


def _long_among_ones():
    rng = _rng(14)
    ones = [_rand(rng, 1) for _ in range(40)]
    return ones[:20] + [_rand(rng, 5000, 4)] + ones[20:] + [_rand(rng, 3, 2)], 8


DEEP_SIZES = [1, 2, 3, 7, 255, 4096, 65537]


def _deep(kind):
    def make():
        if kind == "p2":
            return [_period2(s) for s in DEEP_SIZES], 8
        return [np.full(s, kind, np.uint8) for s in DEEP_SIZES], 8
    return make


def _rand_185000():
    rng = _rng(15)
    return [_rand(rng, 185000) for _ in range(32)], 8


def _text_185000():
    whole = _text(185000 * 32, 5)
    return [whole[i * 185000:(i + 1) * 185000] for i in range(32)], 8


def _rand_1m3():
    rng = _rng(16)
    return [_rand(rng, (1 << 20) + 3) for _ in range(8)], 8


def _k4096():
    rng = _rng(17)
    sizes = rng.integers(1, 301, 4096)
    sizes[:4] = [1, 300, 299, 2]
    return [_rand(rng, int(s), int(rng.integers(1, 5))) for s in sizes], 8


def _starting_points(sp):
    def make():
        rng = _rng(18)
        return [_rand(rng, s, 4) for s in (255, 256, 257, 257, 256, 255)], sp
    return make


CASES = {
    "same_x2": _same(2), "same_x3": _same(3), "same_x64": _same(64),
    "seam_end_begin": _seam_end_begin, "seam_reverse": _seam_reverse,
    "long_among_ones": _long_among_ones,
    "deep_zeros": _deep(0), "deep_ff": _deep(0xFF), "deep_period2": _deep("p2"),
    "rand_185000x32": _rand_185000, "text_185000x32": _text_185000,
    "rand_1m3x8": _rand_1m3,
    "k4096": _k4096,
    "sp1": _starting_points(1), "sp8": _starting_points(8), "sp256": _starting_points(256),
}
SMALL = [n for n in CASES if n not in ("rand_185000x32", "text_185000x32", "rand_1m3x8")]   # what sort_scalar can take too


@functools.lru_cache(maxsize=None)
def case(name):
    blocks, sp = CASES[name]()
    return [np.ascontiguousarray(b, np.uint8) for b in blocks], sp


@functools.lru_cache(maxsize=None)
def model(name):
    blocks, sp = case(name)
    return batchmodel.transform(blocks, sp)


@functools.lru_cache(maxsize=None)
def oracle(name):
    import oracle_lib
    blocks, sp = case(name)
    return [oracle_lib.oracle_bwt_block(b, sp) for b in blocks]


def positions(name):
    """k * S: what the context's max_block_size + 1 has to reach."""
    blocks, _ = case(name)
    return len(blocks) << batchmodel.stride_log2([b.size for b in blocks])


# ---- premises ----------------------------------------------------------------------------------------------------------
def premise(name):
    """Asserts what the case is named for."""
    blocks, sp = case(name)
    sizes = [b.size for b in blocks]
    S = 1 << batchmodel.stride_log2(sizes)
    res = model(name)
    if name.startswith("same_x"):
        assert all((b == blocks[0]).all() for b in blocks) and len(blocks) == int(name[6:])
        assert res["rounds"] >= 1                          # tied inside a block, so the rounds see the copies side by side
        first = res["blocks"][0]
        assert all((o[0] == first[0]).all() and (o[1] == first[1]).all() for o in res["blocks"])
    elif name == "seam_end_begin":
        assert all(s + 1 == S for s in sizes)              # no padding: T_b ends where T_(b+1) begins
        for a, b in zip(blocks[:2], blocks[1:3]):
            assert (a[-400:] == b[:400]).all()             # one block's end is the next block's beginning
        assert (blocks[3] == blocks[4]).all() and not blocks[3].any()
        assert res["rounds"] >= 7                          # repeats of 500 and more: depth 6 * 2^7 is reached
    elif name == "seam_reverse":
        assert all(s + 1 == S for s in sizes)
        assert (blocks[0] == blocks[1][::-1]).all() and (blocks[2] == blocks[3][::-1]).all()
        assert res["rounds"] >= 5
    elif name == "long_among_ones":
        assert sizes.count(1) == 40 and max(sizes) == 5000 and sizes[-1] == 3 and S == 8192
        assert sum(sizes) + len(sizes) < len(sizes) * S // 50      # nearly all positions are padding
    elif name.startswith("deep_"):
        assert sizes == DEEP_SIZES and S == 1 << 17
        # a repeat of 65537 (65536 for period 2) characters: the depth has to pass it, 6 * 2^r >= 65536 -> 14 rounds
        assert res["rounds"] == 14, res["rounds"]
        assert res["active"][0] >= 65537 + 4096 - 12
    elif name in ("rand_185000x32", "text_185000x32"):
        assert sizes == [185000] * 32 and S == 1 << 18
        assert (res["rounds"] >= 3) == (name == "text_185000x32")
    elif name == "rand_1m3x8":
        assert sizes == [(1 << 20) + 3] * 8 and S == 1 << 21      # 2^20 + 3: the stride doubles past 2^20
    elif name == "k4096":
        assert len(blocks) == batchmodel.MAX_BLOCKS and min(sizes) == 1 and max(sizes) == 300 and S == 512
        assert res["rounds"] >= 3
    elif name.startswith("sp"):
        assert sizes[:3] == [255, 256, 257]
        want = {"sp1": [1, 1, 1], "sp8": [1, 1, 8], "sp256": [1, 1, 256]}[name]
        assert [res["blocks"][i][1].size for i in range(3)] == want
        if name == "sp256":
            assert 258 // 256 == 1                        # x = 1: the powers are the rows of suffixes 257, 256, ..., 3
    else:
        raise AssertionError("case %s has no premise" % name)


def random_batch(rng):
    """A small mixed batch for the 100-batch run: sizes, alphabets and block counts all over the place."""
    k = int(rng.choice([1, 2, 3, 5, 17, 64, 130]))
    top = int(rng.choice([1, 8, 40, 300, 3000]))
    blocks = []
    for _ in range(k):
        size = int(rng.integers(1, top + 1))
        sigma = int(rng.choice([1, 2, 3, 16, 256]))
        lo = int(rng.integers(0, 257 - sigma))
        blocks.append((_rand(rng, size, sigma) + lo).astype(np.uint8))
    return blocks, int(rng.choice([1, 8, 256]))
