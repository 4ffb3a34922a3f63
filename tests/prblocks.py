"""Inputs for the pair-replacing pre-stage's limits tests (CPU, numpy only): every builder states a premise about what
the reference's PairReplacer does with its block, tests/test_prblocks.py proves the premise with the oracle alone, and
tests/test_gpu_prepr_limits.py runs the blocks through the device kernels of bwtc_amd/csrc/prepr.hip.

The kernels' grains: a thread takes 16 positions (a "thread seam" is a multiple of 16), a workgroup a tile of 4096
positions (a "tile seam"), the statistics kernel at most 512 workgroups, the run-head scan chunks of 1024 tiles.

What decides a round (PairReplacer::decideReplacements, from an empty grammar): pairs are taken by falling count; a
pair needs a count above 1003 plus the count of the symbol it is given; symbols that do not occur cost nothing and are
used first; when none is left, two rare symbols become special symbols (written doubled) and the next rarest are freed
(written as a pair of special symbols), which pays when the pairs so replaced gain more than 1000.  A pair whose first
byte is 0 is never taken, nor a pair that shares a byte in the other place with a pair already taken."""
import numpy as np

import pgrammar

THREAD, TILE = 16, 4096
A, B, X = 0x62, 0x61, 0x78                                    # the pair AB = "ba" sorts before "ab" at equal counts


def sizes():
    """Block lengths at the minimum, the thread grain, the tile grain, the statistics grid and the head scan's chunk."""
    return [3, 15, 16, 17, 18, 19, 4094, 4095, 4096, 4097, 4098, 4096 + 15, 4096 + 16, 4096 + 17, 4096 + 18,
            8191, 8192, 8193, 512 * 4096 - 1, 512 * 4096 + 1, 513 * 4096 + 17, 1024 * 4096 + 1, 1025 * 4096 + 17]


SMALL = 8193                                                   # sizes up to here run at every alignment


def offsets(n):
    return list(range(16)) if n <= SMALL else [0, 1, 15]


# ---- the counting rule, restated -------------------------------------------------------------------------------

def pair_counts(data):
    """(byte counts[256], pair counts[65536], index first << 8 | second): the pair ending at i counts, except at odd i
    when d[i-2] == d[i-1] == d[i] (with a zero byte before the text)."""
    d = np.ascontiguousarray(data, np.uint8)
    n = d.size
    ext = np.concatenate([np.zeros(1, np.uint8), d])          # ext[i + 1] = d[i]
    i = np.arange(1, n)
    cur, prev, before = ext[i + 1], ext[i], ext[i - 1]
    skip = ((i & 1) == 1) & (before == prev) & (prev == cur)
    pairs = (prev.astype(np.int64) << 8 | cur)[~skip]
    return np.bincount(d, minlength=256).astype(np.uint64), np.bincount(pairs, minlength=65536).astype(np.uint64)


# ---- what a round's output says about its input ------------------------------------------------------------------

def replaced_pairs(raw):
    """The two-byte strings the rules of a serialised grammar stand for (after one round: the pairs it replaced)."""
    rules, specials, freed, _ = pgrammar.read(raw)
    model = pgrammar.expansions(rules, specials, freed)
    return {model.of(var) for var, _ in rules if len(model.of(var)) == 2}


def tokens(raw, out):
    """The tokens of a round's output `out` under the serialised grammar `raw`: (input position each token starts at,
    input bytes it stands for, output bytes it takes)."""
    model = pgrammar.model_of(raw)
    keys, _ = pgrammar.token_keys(model, out)
    in_len = model.key_len[keys]
    out_len = np.where(keys >= 256, 2, 1)
    return np.cumsum(in_len) - in_len, in_len, out_len


def straddled(raw, out):
    """The input positions s such that a replaced pair covers s - 1 and s."""
    start, in_len, _ = tokens(raw, out)
    return set((start[in_len == 2] + 1).tolist())


# ---- pairs_on_seams ------------------------------------------------------------------------------------------

ENDINGS = ("pair", "first", "escape")
_RARE_CHUNKS = 73                                              # 73 threads' interiors of 14 bytes hold the 1009 rare bytes


def seam_limit(n, ending):
    """The seams s <= this are straddled by a pair AB in pairs_on_seams(n, ending)."""
    e = n - {"pair": 2, "first": 3, "escape": 3}[ending]      # where the last whole pair starts
    return n - 1 if e & 1 else e - 2


def pairs_on_seams(n, ending):
    """A then AB AB AB ... (A = "b", B = "a"): the pairs AB start at odd positions, so one covers s - 1 and s for every
    multiple s of 16 (thread seams, tile seams) up to seam_limit; AB occurs at least as often as BA and is tried first
    at equal counts, so it is the pair a round takes when n >= 2100 (BA shares its bytes and cannot follow).  Where the
    ending needs its last pair at an even position, one more B before that pair shifts it.
    The block ends in a whole pair ("pair"), in the pair's first byte with nothing behind it ("first"), or ("escape",
    n >= 4094) in the rarest byte of all: there every other byte value occurs (once, twice, three times, the rest four
    times, inside the threads 1 .. 73 between their straddling pairs), so the round has no unused symbol, makes the two
    rarest ones special symbols and frees the third for AB -- and writes the block's last byte doubled."""
    assert n >= 3 and ending in ENDINGS
    t = np.where(np.arange(n) & 1, A, B).astype(np.uint8)
    t[0] = A
    tail = {"pair": [A, B], "first": [A, B, A], "escape": [A, B, 0]}[ending]
    e = n - len(tail)
    if e < 1:
        t[:] = tail[-n:]
    else:
        t[e:] = tail
        if not e & 1 and e >= 2:
            t[e - 1] = B
    if ending == "escape":
        rest = [c for c in range(256) if c not in (A, B)]
        z0, z1, z2 = rest[-1], rest[-2], rest[-3]
        t[n - 1] = z0
        if n >= 4094:
            rare = [z1] * 2 + [z2] * 3 + [c for c in rest[:-3] for _ in range(4)]
            rare += [rest[0]] * (14 * _RARE_CHUNKS - len(rare))   # fill the last interior with byte 0
            rare = np.array(rare, np.uint8).reshape(_RARE_CHUNKS, 14)
            for k in range(_RARE_CHUNKS):
                t[16 * (k + 1) + 1:16 * (k + 1) + 15] = rare[k]
    return t


# ---- stat_edges ----------------------------------------------------------------------------------------------

QUARTERS = (0, 63, 64, 127, 128, 191, 192, 255)
TRIPLE_AT = (-2, -1, 0, 1)


def stat_edges(n, seed):
    """name -> block of n bytes, made for the counters: two and three symbols at random (triples of equal bytes at both
    parities everywhere), one byte throughout (0: the virtual byte before the text; 0xFF: the last counter of the last
    quarter), a text that starts 00 00 00, the eight bytes at the quarters' edges as first and second byte of a pair,
    and triples of one byte that start at s - 2, s - 1, s and s + 1 for every multiple s of 16."""
    rng = np.random.default_rng(seed * 1000003 + n)
    out = {
        "sigma2": rng.integers(0, 2, n).astype(np.uint8) * 0xC1,
        "sigma3": np.array([0, 0x40, 0xFF], np.uint8)[rng.integers(0, 3, n)],
        "zeros": np.zeros(n, np.uint8),
        "ff": np.full(n, 0xFF, np.uint8),
        "quarters": np.array(QUARTERS, np.uint8)[rng.integers(0, 8, n)],
    }
    s = rng.integers(0, 2, n).astype(np.uint8)
    s[:3] = 0
    out["start000"] = s
    for d in TRIPLE_AT:
        out["triples%+d" % d] = _triples(n, d)
    return out


_TRIPLE_BYTES = (0x00, 0x40, 0x7F, 0xFF)


def _triples(n, d):
    t = np.frombuffer(b"abcdefg" * (n // 7 + 1), np.uint8)[:n].copy()
    for k, s in enumerate(range(THREAD, n + 2, THREAD)):
        if s + d + 3 <= n:
            t[s + d:s + d + 3] = _TRIPLE_BYTES[k & 3]
    return t


def triple_starts(n, d):
    return [s + d for s in range(THREAD, n + 2, THREAD) if s + d + 3 <= n]


# ---- double_runs ---------------------------------------------------------------------------------------------

WHERE = ("start-1", "start+0", "start+1", "end-1", "end+0", "end+1", "through")
_GAP = np.array([0x63, 0x64, 0x65, 0x66], np.uint8)


def _run_template(where):
    """4096 bytes around a tile seam (the seam is position 2048 of them): runs of X between thread seams, each starting
    at a seam - 1, + 0 or + 1 and ending (exclusive) at a later seam - 1, + 0 or + 1 -- all nine combinations in turn, so
    both parities of length -- with 13 to 17 other bytes between two runs; at the tile seam itself the event `where`."""
    rng = np.random.default_rng(7)
    t = _GAP[rng.integers(0, 4, TILE)]
    kind, at = (where[:-2], int(where[-2:])) if where != "through" else ("through", 0)
    runs = []                                                  # (first position, position behind the last)
    centre = TILE // 2
    if kind == "start":
        runs.append((centre + at, centre + 48 + 1))
    elif kind == "end":
        runs.append((centre - 48 - 1, centre + at))
    else:
        runs.append((centre - 48 + 1, centre + 48 - 1))
    combos = [(ds, de) for ds in (-1, 0, 1) for de in (-1, 0, 1)]
    k = 0
    s = 32
    while s + 80 < TILE:
        m = 2 + k % 3
        ds, de = combos[k % 9]
        a, b = s + ds, s + THREAD * m + de
        if b + 20 < runs[0][0] or a - 20 > runs[0][1]:
            runs.append((a, b))
            k += 1
        s += THREAD * (m + 1)
    for a, b in runs:
        t[a:b] = X
    return t, sorted(runs)


def double_runs(n, where):
    """The template of `where`, repeated so that its middle lies on every tile seam.  X is most of the text, so for
    n >= 4094 "XX" is the most frequent pair by far and the round replaces it (no other pair with an X can follow it)."""
    t, _ = _run_template(where)
    reps = (n + TILE // 2) // TILE + 2
    return np.tile(t, reps)[TILE // 2:TILE // 2 + n].copy()


LONG_RUN = 1024 * 4096 + 4096 + 3
LONG_RUN_START = 1237                                          # odd, inside tile 0


def long_double_run():
    """Other text, then from position 1237 a run of 1024 * 4096 + 4096 + 3 bytes of X: it reaches over all of the head
    scan's first chunk of 1024 tiles into the second, where only the chunk's carry says where it started -- at an odd
    position, so a run taken to start at 0 pairs its bytes the other way round.  Other text and short runs follow."""
    rng = np.random.default_rng(11)
    n = LONG_RUN_START + LONG_RUN + 3 * TILE + 5
    t = _GAP[rng.integers(0, 4, n)]
    t[LONG_RUN_START:LONG_RUN_START + LONG_RUN] = X
    tail = LONG_RUN_START + LONG_RUN
    for k in range(6):
        a = tail + 700 + 1001 * k
        t[a:a + 6 + k] = X
    return t


def run_at_tile_1024():
    """1025 * 4096 + 17 bytes: other text with short runs of X, and a run of X from the first position of tile 1024 (the
    first tile of the head scan's second chunk) to 30 bytes before the end."""
    rng = np.random.default_rng(12)
    n = 1025 * TILE + 17
    t = np.tile(double_runs(4 * TILE, "through"), 1024 // 4 + 1)[:n].copy()
    first = 1024 * TILE
    t[first - 40:first] = _GAP[rng.integers(0, 4, 40)]
    t[first:n - 30] = X
    t[n - 30:] = _GAP[rng.integers(0, 4, 30)]
    return t


# ---- one_count_decides ---------------------------------------------------------------------------------------

P = (250, 251)
DECIDE_TILES = 64


def _background(rng, n):
    t = rng.integers(1, 201, n).astype(np.uint8)              # 200 symbols: a pair occurs some six times in 64 tiles
    t[t == X] = 201
    return t


def one_count_decides(k):
    """64 tiles of random bytes 1 .. 201 (without X) and the pair P = (250, 251) exactly k times: once over each of the 63 tile
    seams, the rest over thread seams.  56 byte values do not occur, so a symbol for P costs nothing and the round
    takes P exactly when k > 1003; no other pair comes near."""
    rng = np.random.default_rng(21)
    n = DECIDE_TILES * TILE
    t = _background(rng, n)
    seams = [TILE * i for i in range(1, DECIDE_TILES)]
    free = np.array([s for s in range(THREAD, n, THREAD) if s % TILE])
    seams += sorted(rng.choice(free, k - len(seams), replace=False).tolist())
    for s in seams:
        t[s - 1], t[s] = P
    return t


def one_count_decides_double(k):
    """The same for the pair XX, counted through the rule for three equal bytes: "XXX" from an even position counts
    twice (pairs ending at odd and even positions), from an odd position once (the pair ending at the odd position
    two behind is the same pair again).  Triples start at s - 2 and s - 1 of tile seams (alternating) and of thread
    seams; their counts add up to exactly k."""
    rng = np.random.default_rng(22)
    n = DECIDE_TILES * TILE
    t = _background(rng, n)
    total = 0
    tile_seams = [TILE * i for i in range(1, DECIDE_TILES)]
    free = rng.permutation(np.array([s for s in range(THREAD, n, THREAD) if s % TILE])).tolist()
    for i, s in enumerate(tile_seams + free):
        if total == k:
            break
        even = (i & 1) == 0 and total + 2 <= k
        a = s - 2 if even else s - 1
        t[a:a + 3] = X
        total += 2 if even else 1
    assert total == k
    return t


# ---- all_escaped_tile ----------------------------------------------------------------------------------------

RAREST = (1, 2, 3, 4)
FREQUENT = ((0x41, 0x42), (0x43, 0x44))


def all_escaped_tile():
    """Tile 0: the bytes 1, 2, 3 and 4, 1024 times each, shuffled (their sixteen pairs occur some 256 times each).
    Behind it every other byte value 1200 times, shuffled, with "AB" and "CD" written over it 2600 times each.  No
    symbol is unused, the four of tile 0 are the rarest, and 2600 + 2600 - 4 * 1024 > 1000: the round makes two of them
    special symbols and frees the other two for "AB" and "CD", so each of tile 0's 4096 positions is written as two
    special bytes -- a tile's largest output, 8192 bytes."""
    rng = np.random.default_rng(31)
    tile0 = rng.permutation(np.repeat(np.array(RAREST, np.uint8), TILE // 4))
    others = np.array([c for c in range(256) if c not in RAREST], np.uint8)
    rest = rng.permutation(np.repeat(others, 1200))
    slots = rng.choice(rest.size // 2 - 1, 5200, replace=False) * 2 + 1
    for i, a in enumerate(slots.tolist()):
        rest[a:a + 2] = FREQUENT[i & 1]
    return np.concatenate([tile0, rest])


# ---- rounds_to_exhaustion ------------------------------------------------------------------------------------

ROUNDS_CAP = 16


def rounds_to_exhaustion(seed):
    """1 MiB of text: 40 words of 8 to 23 letters over an alphabet of eight, drawn with slowly falling probability.
    Round after round finds frequent pairs among the symbols the rounds before made; from the fourth round on the unused
    byte values are spent, so special symbols multiply and the pairs that touch them are barred."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"etaoinsh", np.uint8)
    words = [bytes(letters[rng.integers(0, letters.size, int(rng.integers(8, 24)))]) + b" " for _ in range(40)]
    p = 1.0 / np.sqrt(np.arange(1, 41))
    pick = rng.choice(40, 140000, p=p / p.sum())
    text = b"".join(words[int(i)] for i in pick)
    assert len(text) >= 1 << 20
    return np.frombuffer(text[:1 << 20], np.uint8).copy()
