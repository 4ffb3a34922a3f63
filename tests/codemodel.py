"""Test-side model of the suffix sorter's code-key stage (k_pair_counts, k_code_build,
k_make_keys_code in bwtc_amd/csrc/bwt_engine.hip), the part tests/sortmodel.py plays for the radix sorts: plain numpy
and Python integers, nothing of bwtc_amd.

Five things are restated: the dense codes of plan_keys (lut_of), the sampled pair counts (pair_counts), the
weight-balanced alphabetic code table (build_table), and the keys, second words, plane bytes and levels (make_keys).
Two properties come from first principles instead -- sorted() over the padded dense-code strings (suffix_order):
  monotone   along the true suffix order the key's value never decreases (monotone_breaks);
  level      suffixes with equal values carry the same level and share at least level_depth(level) leading dense
             codes (level_breaks).
cases() lists the named cases tests/test_gpu_code_keys.py runs, each a small dict with a fixed seed; make() draws a
case's input, expected() is the model's answer, properties() says from the drawn input which edges the case reaches
(tests/test_codemodel.py holds every case to the edges it is named for)."""
import bisect

import numpy as np

PAD = 128                       # kTextPad: zero bytes behind T
PAIR_TILE = 4096                # kPairTile
MAX_GROUPS = 512                # sampled tiles at most
MAX_LEN = 26                    # kCodeMaxLen
ORDER0 = 256                    # kCodeOrder0: the table's order-0 row
MAX_PAIRS = 1 << 21             # 512 tiles of 4096 pairs
LEVEL_MIN = (1, 8, 12, 16, 20, 24, 32, 48)      # code_level_depth(level); code_level_of(k) = the last level with LEVEL_MIN <= k
WINDOW = PAD                    # dense codes of a suffix the first-principles order compares (a key sees at most 72)
U64 = np.uint64


def level_of(k):
    return np.searchsorted(np.array(LEVEL_MIN[1:]), np.asarray(k), side="right")


def level_depth(level):
    return np.array(LEVEL_MIN)[np.asarray(level)]


# ---- the dense codes -----------------------------------------------------------------------------------------------
def lut_of(T, lone_sentinel):
    """plan_keys: lut[c] = the number of present byte values below c (at most 255), sigma = max(2, present values).
    lone_sentinel: the zero byte (the terminator alone) is not present and shares code 0 with the smallest symbol."""
    present = np.bincount(np.asarray(T, np.uint8), minlength=256) > 0
    if lone_sentinel:
        present[0] = False
    lut = np.minimum(np.cumsum(present) - present, 255).astype(np.uint8)
    return lut, max(2, int(present.sum()))


def padded_codes(T, lut):
    """Dense codes of T and of the PAD zero bytes behind it."""
    return np.concatenate([np.asarray(lut)[np.asarray(T, np.uint8)], np.full(PAD, lut[0], np.uint8)])


# ---- the pair counts -----------------------------------------------------------------------------------------------
def sampled_tiles(n):
    ntiles = -(-n // PAIR_TILE)
    groups = min(ntiles, MAX_GROUPS)
    return [b * ntiles // groups for b in range(groups)]


def pair_counts(T, lut):
    """counts[a, b] of the pairs (code(T[j-1]), code(T[j])), 0 < j < n, j in a sampled tile."""
    T = np.asarray(T, np.uint8)
    n = T.size
    code = np.asarray(lut)[T].astype(np.int64)
    cnt = np.zeros(65536, np.int64)
    for t in sampled_tiles(n):
        a, b = max(1, t * PAIR_TILE), min(n, (t + 1) * PAIR_TILE)
        if b > a:
            cnt += np.bincount(code[a - 1:b - 1] * 256 + code[a:b], minlength=65536)
    return cnt.reshape(256, 256).astype(np.uint32)


# ---- the code table ------------------------------------------------------------------------------------------------
_ROWS = {}


def build_row(c, sigma):
    """One row of k_code_build over the counts c[0 .. sigma) -> (256 entries len << 27 | bits, the longest length)."""
    c = [int(x) for x in c[:sigma]]
    total, sh = sum(c), 0
    while (total >> sh) >= 65536:
        sh += 1
    wt = tuple((x >> sh) + 1 for x in c)
    hit = _ROWS.get(wt)
    if hit is not None:
        return hit
    pre2 = [0]                                   # doubled prefix sums of the weights
    for x in wt:
        pre2.append(pre2[-1] + 2 * x)
    out, longest = [0] * 256, 0
    stack = [(0, sigma, 0, 0)]
    while stack:
        lo, hi, bits, ln = stack.pop()
        if hi - lo > 1 and ln <= 31:
            mid2 = (pre2[lo] + pre2[hi]) // 2    # the interval's doubled midpoint
            cut = bisect.bisect_left(pre2, mid2, lo + 1, hi - 1)      # the smallest cut that reaches it, else hi - 1
            if cut > lo + 1:
                da = abs(pre2[cut] - mid2)
                db = mid2 - pre2[cut - 1]
                if db <= da:                     # one left when that is at least as close
                    cut -= 1
            stack.append((lo, cut, bits << 1, ln + 1))
            stack.append((cut, hi, (bits << 1) | 1, ln + 1))
        else:
            ln = max(ln, 1)                      # (an alphabet of one symbol)
            longest = max(longest, ln)
            for s in range(lo, hi):
                out[s] = ((ln << 27) | bits) & 0xFFFFFFFF
    _ROWS[wt] = (out, longest)
    return out, longest


def build_table(counts, sigma):
    """-> (table[257, 256], the error word: 2 when a codeword is longer than MAX_LEN).  Row 256 is the order-0 row:
    the counts summed over the contexts below sigma."""
    counts = np.asarray(counts).reshape(256, 256).astype(np.int64)
    table, longest = np.zeros((257, 256), np.uint32), 0
    for row in range(257):
        c = counts[row] if row < 256 else counts[:sigma].sum(axis=0)
        out, ln = build_row(c, sigma)
        table[row] = out
        longest = max(longest, ln)
    return table, (2 if longest > MAX_LEN else 0)


def row_checks(row, sigma):
    """A row's truths: dict(lengths ok, prefix free, alphabetic, kraft numerator over 2^32 == 2^32, longest)."""
    ln = [int(e) >> 27 for e in row[:sigma]]
    bits = [int(e) & 0x7FFFFFF for e in row[:sigma]]
    ok = all(1 <= l <= 31 and b >> l == 0 for l, b in zip(ln, bits))
    left = [b << (32 - l) for l, b in zip(ln, bits)]                        # left-aligned in 32 bits
    ends = [a + (1 << (32 - l)) for a, l in zip(left, ln)]                  # one behind the codeword's subtree
    alphabetic = all(left[s] < left[s + 1] for s in range(sigma - 1))
    order = sorted(range(sigma), key=lambda s: (left[s], ln[s]))
    prefix_free = all(ends[order[i]] <= left[order[i + 1]] for i in range(sigma - 1))
    kraft = sum(1 << (32 - l) for l in ln)
    return dict(ok=ok and not any(int(e) for e in row[sigma:]), prefix_free=prefix_free, alphabetic=alphabetic,
                complete=kraft == 1 << 32 or (sigma == 1 and kraft == 1 << 31), longest=max(ln))


def table_checks(table, sigma):
    """row_checks over all 257 rows, and-ed; longest = the longest codeword of the table."""
    table = np.asarray(table).reshape(257, 256)
    res, seen = dict(ok=True, prefix_free=True, alphabetic=True, complete=True, longest=0), {}
    for row in table:
        key = row.tobytes()
        if key not in seen:
            seen[key] = row_checks(row, sigma)
        r = seen[key]
        for f in ("ok", "prefix_free", "alphabetic", "complete"):
            res[f] = res[f] and r[f]
        res["longest"] = max(res["longest"], r["longest"])
    return res


# ---- the keys ------------------------------------------------------------------------------------------------------
def key_layout(kbits, split):
    hi_shift = kbits - 32
    chr_shift = hi_shift + (13 if split else 0)
    return hi_shift, chr_shift, chr_shift + 8


def make_keys(T, lut, table, kbits, split):
    """-> dict: keys, w, plane as the kernel leaves them (slot j for suffix n - 1 - j), and per suffix (index = suffix)
    hi, lo (the value's upper kbits - 32 and lower 32 bits), level, k (complete codewords), need, and used_len (the
    lengths of the codewords that make up the block's bit string)."""
    T = np.asarray(T, np.uint8)
    table = np.asarray(table).reshape(257, 256)
    n = T.size
    code = padded_codes(T, lut).astype(np.int64)
    ent = table[code[:-1], code[1:]].astype(np.int64)      # ent[j - 1]: position j in the context of position j - 1
    ln, cw = ent >> 27, ent & 0x7FFFFFF
    start = np.concatenate([[0], np.cumsum(ln)])           # start[j - 1]: the bit where position j's codeword begins
    total = int(start[-1])
    bit = np.zeros(total + 2 * PAD, np.uint8)
    end = np.zeros(total + 2 * PAD, np.int64)
    for b in range(int(ln.max()) if ln.size else 0):
        m = ln > b
        bit[start[:-1][m] + b] = (cw[m] >> (ln[m] - 1 - b)) & 1
    end[(start[:-1] + ln - 1)[ln > 0]] = 1
    ends_before = np.concatenate([[0], np.cumsum(end)])
    first = table[ORDER0, code[:n]].astype(np.int64)
    l0, fc = first >> 27, first & 0x7FFFFFF
    need = kbits - l0
    s0 = start[:n]                                         # suffix i reads from position i + 1 on
    hi, lo = np.zeros(n, U64), np.zeros(n, U64)
    for p in range(kbits):
        b = np.where(p < l0, (fc >> np.maximum(l0 - 1 - p, 0)) & 1, bit[s0 + np.maximum(p - l0, 0)]).astype(U64)
        if p < kbits - 32:
            hi = (hi << U64(1)) | b
        else:
            lo = (lo << U64(1)) | b
    k = 1 + ends_before[s0 + need] - ends_before[s0]
    level = level_of(k)
    i = np.arange(n, dtype=np.int64)
    prev = np.concatenate([[0], code[:n - 1]]) if n else code[:0]
    hi_shift, chr_shift, lvl_shift = key_layout(kbits, split)
    keys = hi | (prev.astype(U64) << U64(chr_shift)) | (level.astype(U64) << U64(lvl_shift))
    if split:
        keys |= (i >> 16).astype(U64) << U64(hi_shift)
    w = lo.astype(np.uint32)
    return dict(keys=keys[::-1].copy(), w=w[::-1].copy(), plane=(w & np.uint32(255)).astype(np.uint8)[::-1].copy(),
                hi=hi, lo=lo, level=level, k=k, need=need, used_len=ln[:max(n - 1, 0) + 72])


def unpack(keys, w, kbits, split):
    """Device arrays (slot order) -> per suffix (hi, lo, level): what the two properties are asked of."""
    hi_shift, chr_shift, lvl_shift = key_layout(kbits, split)
    keys = np.asarray(keys, U64)[::-1]
    return keys & U64((1 << hi_shift) - 1), np.asarray(w)[::-1].astype(U64), ((keys >> U64(lvl_shift)) & U64(7)).astype(np.int64)


# ---- first principles ----------------------------------------------------------------------------------------------
def windows(T, lut):
    code = np.concatenate([padded_codes(T, lut), np.full(WINDOW, lut[0], np.uint8)])
    return np.lib.stride_tricks.sliding_window_view(code, WINDOW)[:np.asarray(T).size]


def suffix_order(T, lut):
    """The suffixes by their padded dense-code strings: sorted(), nothing of the code table."""
    win = windows(T, lut)
    return np.array(sorted(range(win.shape[0]), key=lambda i: win[i].tobytes()), np.int64)


def monotone_breaks(order, hi, lo):
    """Places of the true order where the value (hi, lo) decreases."""
    h, l = hi[order], lo[order]
    return int(((h[1:] < h[:-1]) | ((h[1:] == h[:-1]) & (l[1:] < l[:-1]))).sum())


def level_breaks(order, hi, lo, level, T, lut):
    """Neighbours in the true order with equal values whose levels differ or that share fewer than
    level_depth(level) leading dense codes (equal values are neighbours once the order is monotone)."""
    h, l, lv = hi[order], lo[order], level[order]
    same = np.flatnonzero((h[1:] == h[:-1]) & (l[1:] == l[:-1]))
    if same.size == 0:
        return 0
    win = windows(T, lut)
    eq = win[order[same]] == win[order[same + 1]]
    lcp = np.where(eq.all(axis=1), WINDOW, np.argmin(eq, axis=1))
    return int(((lv[same] != lv[same + 1]) | (lcp < level_depth(lv[same]))).sum())


# ---- tables of the key-maker cases ---------------------------------------------------------------------------------
def fixed_table(sigma, l0, L):
    """Order-0 codewords of l0 bits, context codewords of L bits: symbol s is the number s."""
    assert sigma <= 1 << min(l0, L)
    t = np.zeros((257, 256), np.uint32)
    t[:256, :sigma] = (L << 27) | np.arange(sigma)
    t[256, :sigma] = (l0 << 27) | np.arange(sigma)
    return t


def comb_table(sigma):
    """1-bit and 26-bit codewords: symbol 0 is '0', symbol s > 0 is '1' and s in 25 bits."""
    t = np.zeros((257, 256), np.uint32)
    t[:, 1:sigma] = (26 << 27) | (1 << 25) | np.arange(1, sigma)
    t[:, 0] = 1 << 27
    return t


TABLES = {
    "onebit": lambda: (2, fixed_table(2, 1, 1)),          # 71 codewords behind the first: the whole look-ahead, level 7
    "all26": lambda: (256, fixed_table(256, 26, 26)),     # the tile's bit string at its fullest, level 0
    "mixed": lambda: (16, comb_table(16)),                # codewords straddle the 32-bit words at every offset
}


def level_pair(kbits, target):
    """(l0, L) with 1 + (kbits - l0) // L == target, the largest alphabet first."""
    best = None
    for L in range(1, 27):
        for l0 in range(1, 27):
            if 1 + (kbits - l0) // L == target and (best is None or min(l0, L) > min(best)):
                best = (l0, L)
    return best


# ---- texts ---------------------------------------------------------------------------------------------------------
def structured_text(rng, n, sigma, zeros):
    """Words over `sigma` byte values with planted repeats, a periodic stretch and a run (the generator of
    test_long_key_route_on_small_structured_blocks, cut down); zeros: the zero byte is one of the values."""
    alphabet = rng.choice(np.arange(1, 256), sigma, replace=False).astype(np.uint8)
    if zeros:
        alphabet[0] = 0
    words = [alphabet[rng.integers(0, sigma, int(rng.integers(1, 9)))] for _ in range(int(rng.integers(5, 200)))]
    d = np.concatenate([words[int(i)] for i in rng.integers(0, len(words), n // 3 + 8)])
    d = np.concatenate([d, alphabet])[:n].copy() if d.size < n else d[:n].copy()
    for _ in range(8):                                      # planted repeats
        ln = int(min(n // 3, rng.integers(1, 1 + int(rng.choice([40, 2000])))))
        a, b = int(rng.integers(0, n - ln)), int(rng.integers(0, n - ln))
        d[b:b + ln] = d[a:a + ln].copy()
    p = d[:int(rng.integers(1, 30))].copy()                 # a periodic stretch
    a, ln = int(rng.integers(0, n // 2)), int(rng.integers(200, n // 4))
    d[a:a + ln] = np.tile(p, ln // p.size + 1)[:ln]
    a = int(rng.integers(0, n - 400))
    d[a:a + 300] = alphabet[-1]                             # a run
    d[:sigma] = alphabet                                    # every symbol is there
    return d


SEAM_BYTES = dict(tile=(201, 202), thread=(203, 204), first=205, last=206)


def seam_text(rng, n, lone):
    """Six common byte values, and pairs that occur nowhere else across every seam of the pair counter: (201, 202)
    across the 4096 tile seams, (203, 204) across every fifth 16-byte thread seam, 205 at position 0, 206 at position
    n - 1 (lone: the terminator's zero byte there, the text's only one; else zero is one of the common values)."""
    base = np.array([0 if not lone else 9, 10, 11, 12, 13, 14], np.uint8)
    T = base[rng.integers(0, base.size, n)]
    j = np.arange(16, n, 16)
    j = j[(j // 16) % 5 == 3]
    T[j - 1], T[j] = SEAM_BYTES["thread"]
    j = np.arange(PAIR_TILE, n, PAIR_TILE)
    T[j - 1], T[j] = SEAM_BYTES["tile"]
    T[0] = SEAM_BYTES["first"]
    T[n - 1] = 0 if lone else SEAM_BYTES["last"]
    return T


# ---- named cases ---------------------------------------------------------------------------------------------------
COUNT_N = (1, 2, 15, 16, 17, 4095, 4096, 4097, 8 * 4096 + 5, 511 * 4096 + 3, 512 * 4096, 513 * 4096 + 7, 1500 * 4096 + 1)
KEYS_UP_TO = 70000                                      # the whole-stage cases compare keys up to here
TABLE_SIGMA = (1, 2, 3, 4, 255, 256)
TABLE_KINDS = ("zeros", "one_big", "totals", "equal", "deep", "ends")
KEY_N = (1, 2, 3, 1023, 1024, 1025, 2049, 65536 + 1025)
KEY_BITS = (40, 41, 63, 64, 65, 71, 72)
LEVEL_TARGETS = (7, 8, 11, 12, 15, 16, 19, 20, 23, 24, 31, 32, 47, 48)
STAGE_SIGMA = (2, 20, 60, 230)
STAGE_BITS = (40, 48, 72)
STAGE_N = (5003, 20481, 60000)


def _key_case(bucket, tname, n, kbits, text, split=True, table=None, edge=None):
    return dict(form="keys", group="keys", bucket=bucket, table=tname, tparm=table, n=n, kbits=kbits, text=text, split=split,
                edge=edge or {}, name="keys-%s-%s-n%d-k%d-%s-%s" % (bucket, tname, n, kbits, text, "split" if split else "whole"))


def _key_cases():
    out = []
    for tname in TABLES:
        edge = {"onebit": dict(longest=1), "all26": dict(longest=26, levels=(0,)), "mixed": dict(longest=26, offsets=32)}[tname]
        for n in KEY_N:
            for kbits in KEY_BITS:
                e = dict(edge, key_tiles=-(-n // 1024), key_rem=n % 1024)
                if tname == "onebit":
                    e.update(levels=(int(level_of(kbits)),), k=(kbits,))
                if tname == "mixed" and n < 1023:
                    e = dict(key_tiles=e["key_tiles"], key_rem=e["key_rem"])
                if n > 65536:
                    e.update(upper_bits=True)
                out.append(_key_case("sizes-" + tname, tname, n, kbits, "random", edge=e))
                if n > 65536:
                    out.append(_key_case("sizes-" + tname, tname, n, kbits, "random", split=False, edge=e))
        for text in ("same", "tail80", "lone"):
            for kbits in (40, 65, 72):
                for n in (1025, 2049):
                    out.append(_key_case("texts-" + tname, tname, n, kbits, text, edge=dict(text_ok=True)))
    for target in LEVEL_TARGETS:
        made = 0
        for kbits in (72, 41):
            pair = level_pair(kbits, target)
            if pair:
                made += 1
                out.append(_key_case("levels", "fixed_%d_%d" % pair, 2049, kbits, "random", table=pair, edge=dict(k=(target,))))
        assert made
    for l0 in range(9, 27):                               # need = 14 .. 31: the branch below 32
        out.append(_key_case("need", "fixed_%d_3" % l0, 2049, 40, "random", table=(l0, 3), edge=dict(need=(40 - l0,), below32=2049)))
    out.append(_key_case("need", "fixed_8_3", 2049, 40, "random", table=(8, 3), edge=dict(need=(32,), need32=2049)))
    out.append(_key_case("need", "fixed_8_3", 2049, 72, "random", table=(8, 3), edge=dict(need=(64,), need64=2049)))
    for l0 in range(1, 8):                                # need = 65 .. 71
        out.append(_key_case("need", "fixed_%d_3" % l0, 2049, 72, "random", table=(l0, 3), edge=dict(need=(72 - l0,), above64=2049)))
    return out


def _cases():
    out = []
    for n in COUNT_N:
        for lone in (False, True):
            ntiles = -(-n // PAIR_TILE)
            out.append(dict(form="stage", group="counts", bucket="n%d" % n, n=n, lone=lone, kbits=72, split=True, text="seams",
                            want_keys=n <= KEYS_UP_TO, name="counts-n%d-%s" % (n, "lone" if lone else "zero"),
                            edge=dict(tiles=ntiles, sampled=min(ntiles, MAX_GROUPS), partial=n % PAIR_TILE != 0, skips=ntiles > MAX_GROUPS,
                                      seams=n > 4097)))
    for sigma in TABLE_SIGMA:
        for kind in TABLE_KINDS:
            out.append(dict(form="table", group="table", bucket="sigma%d" % sigma, sigma=sigma, kind=kind, edge=dict(kind_ok=True),
                            name="table-sigma%d-%s" % (sigma, kind)))
    out += _key_cases()
    i = 0
    for sigma in STAGE_SIGMA:
        for zeros in (True, False):
            for kbits in STAGE_BITS:
                n = STAGE_N[i % 3]
                out.append(dict(form="stage", group="stage", bucket="sigma%d" % sigma, n=n, lone=not zeros, kbits=kbits, split=i % 4 != 3,
                                text="structured", sigma=sigma, want_keys=True, edge=dict(sigma=max(2, sigma)),
                                name="stage-sigma%d-%s-k%d-n%d" % (sigma, "zeros" if zeros else "lone", kbits, n)))
                i += 1
    return out


_CASES = None


def cases(group=None):
    global _CASES
    if _CASES is None:
        _CASES = _cases()
        for i, c in enumerate(_CASES):
            c["seed"] = 7919 * i + 29
        assert len({c["name"] for c in _CASES}) == len(_CASES)
    return [c for c in _CASES if group is None or c["group"] == group]


def buckets(group):
    seen = []
    for c in cases(group):
        if c["bucket"] not in seen:
            seen.append(c["bucket"])
    return seen


# ---- a case's input ------------------------------------------------------------------------------------------------
def _weights_row(kind, sigma, rng, which):
    """One row of counts for a table case; `which` picks the row's variant."""
    c = np.zeros(256, np.int64)
    if kind == "totals":                                  # a row total of 65535 (shift 0) and one of 65536 (shift 1)
        total = 65535 + which
        cuts = np.sort(rng.integers(0, total + 1, sigma - 1))
        c[:sigma] = np.diff(np.concatenate([[0], cuts, [total]]))
    elif kind == "deep":                                  # geometric and Fibonacci weights, ascending and descending
        seq, a, b = [], 1, 1                              # (rows 0, 1: doubling; 2, 3: Fibonacci; 4: tripling)
        while sum(seq) + a <= 65535:
            seq.append(a)
            a, b = (2 * a, b) if which < 2 else (b, a + b) if which < 4 else (3 * a, b)
        seq = seq[:sigma]
        row = np.zeros(sigma, np.int64)
        row[sigma - len(seq):] = seq
        c[:sigma] = row[::-1] if which % 2 else row
    elif kind == "ends":                                  # the weight entirely at the last symbol, or at the first
        c[sigma - 1 if which == 0 else 0] = 50000
    return c


def make(c):
    """The case's input: a dict of arrays (the same every time)."""
    rng = np.random.default_rng(c["seed"])
    if c["form"] == "table":
        sigma, kind = c["sigma"], c["kind"]
        counts = np.zeros((256, 256), np.int64)
        if kind == "one_big":
            counts[sigma // 2, sigma // 3] = MAX_PAIRS
        elif kind == "equal":                             # ties at every cut
            counts[:, :] = 3
        elif kind != "zeros":
            for row in range({"totals": 2, "deep": 5, "ends": 2}[kind]):
                counts[row] = _weights_row(kind, sigma, rng, row)
        assert int(counts.sum()) <= MAX_PAIRS
        return dict(counts=counts.astype(np.uint32))
    n = c["n"]
    if c["form"] == "stage":
        if c["text"] == "seams":
            return dict(T=seam_text(rng, n, c["lone"]))
        T = structured_text(rng, n, c["sigma"], not c["lone"])
        if c["lone"]:
            T[n - 1] = 0
        return dict(T=T)
    sigma, table = TABLES[c["table"]]() if c["tparm"] is None else (min(256, 1 << min(c["tparm"])), None)
    if table is None:
        table = fixed_table(sigma, *c["tparm"])
    shift = 1 if c["text"] == "lone" else 0               # lone: bytes 1 .. sigma, the terminator shares code 0 with byte 1
    lut = np.clip(np.arange(256) - shift, 0, sigma - 1).astype(np.uint8)
    if c["table"] == "mixed":                             # half the characters take the 1-bit codeword
        sym = np.where(rng.integers(0, 2, n) == 0, 0, rng.integers(0, sigma, n))
    else:
        sym = rng.integers(0, sigma, n)
    if c["text"] in ("same", "tail80"):
        sym[:] = sigma - 1
    if c["text"] == "tail80":                             # the last 80 positions differ: the padding's codewords are in the last keys
        sym[-80:] = rng.integers(0, sigma, 80)
        sym[-1] = max(1, sigma - 2)
    T = (np.minimum(sym, 255 - shift) + shift).astype(np.uint8)
    if c["text"] == "lone":
        T[n - 1] = 0
    return dict(T=T, lut=lut, sigma=sigma, table=table)


def expected(c, inp):
    """The model's answer: table cases dict(table, err); key cases make_keys(); stage cases the chained model --
    lut, sigma, counts, table, err and (want_keys) the keys."""
    if c["form"] == "table":
        table, err = build_table(inp["counts"], c["sigma"])
        return dict(table=table, err=err)
    if c["form"] == "keys":
        return make_keys(inp["T"], inp["lut"], inp["table"], c["kbits"], c["split"])
    lut, sigma = lut_of(inp["T"], c["lone"])
    counts = pair_counts(inp["T"], lut)
    table, err = build_table(counts, sigma)
    out = dict(lut=lut, sigma=sigma, counts=counts, table=table, err=err)
    if c["want_keys"]:
        out.update(make_keys(inp["T"], lut, table, c["kbits"], c["split"]))
    return out


# ---- what a drawn input reaches ------------------------------------------------------------------------------------
def _key_properties(c, T, exp):
    n = T.size
    k, need = exp["k"], exp["need"]
    used = exp["used_len"]
    starts = np.concatenate([[0], np.cumsum(used)])[:-1]
    long_ = used == MAX_LEN
    return dict(key_tiles=-(-n // 1024), key_rem=n % 1024, longest=int(used.max()) if used.size else 0,
                need=tuple(sorted(set(need.tolist()))), below32=int((need <= 31).sum()), need32=int((need == 32).sum()),
                need64=int((need == 64).sum()), above64=int(((need >= 65) & (need <= 71)).sum()),
                k=tuple(sorted(set(k.tolist()))), levels=tuple(sorted(set(exp["level"].tolist()))),
                k_hist={int(v): int((k == v).sum()) for v in set(k.tolist())},
                offsets=int(np.unique(starts[long_] % 32).size), straddles=int(((starts % 32) + used > 32).sum()),
                upper_bits=n > 65536)


def properties(c, inp, exp=None):
    """Edges the drawn input reaches, by name (see the `edge` dict of every case)."""
    exp = expected(c, inp) if exp is None else exp
    if c["form"] == "table":
        sigma, counts = c["sigma"], inp["counts"].astype(np.int64)
        chk = table_checks(exp["table"], sigma)
        tot = counts[:, :sigma].sum(axis=1)
        lens = (exp["table"][:, :sigma] >> 27).astype(np.int64)
        floor_lg, ceil_lg = max(1, sigma.bit_length() - 1), max(1, (sigma - 1).bit_length())
        kind_ok = {"zeros": int(lens.min()) >= floor_lg and int(lens.max()) <= ceil_lg,
                   "one_big": int(counts.max()) == MAX_PAIRS and int((counts > 0).sum()) == 1,
                   "totals": int(tot[0]) == 65535 and int(tot[1]) == 65536,
                   "equal": np.unique(counts).size == 1 and int(counts[0, 0]) > 0,
                   "deep": int((counts.sum(axis=1) > 0).sum()) == 5 and int(tot.max()) <= 65535,
                   "ends": int(counts[0, sigma - 1]) > 0 and int(counts[1, 0]) > 0 and int((counts > 0).sum()) <= 2}[c["kind"]]
        return dict(kind_ok=kind_ok, longest=chk["longest"], err=exp["err"], checks=chk)
    T = inp["T"]
    n = T.size
    if c["form"] == "keys":
        p = _key_properties(c, T, exp)
        sym = inp["lut"][T]
        p["text_ok"] = {"random": True, "same": np.unique(sym).size == 1,
                        "tail80": np.unique(sym[:-80]).size == 1 and np.unique(sym[-80:]).size > 1 and sym[-1] != 0,
                        "lone": T[n - 1] == 0 and not (T[:-1] == 0).any() and inp["lut"][0] == inp["lut"][1] == 0}[c["text"]]
        return p
    ntiles = -(-n // PAIR_TILE)
    tiles = sampled_tiles(n)
    p = dict(tiles=ntiles, sampled=len(tiles), partial=n % PAIR_TILE != 0, skips=len(tiles) < ntiles, sigma=exp["sigma"],
             distinct_tiles=len(set(tiles)) == len(tiles), lone_ok=(not c["lone"]) or (T[n - 1] == 0 and not (T[:-1] == 0).any()),
             merged=bool(c["lone"] and exp["lut"][0] == 0 and exp["lut"][T[T > 0].min()] == 0) if n > 1 else None)
    if c["text"] == "seams":
        code = exp["lut"].astype(np.int64)
        cnt = exp["counts"]
        t1, t2 = SEAM_BYTES["tile"]
        h1, h2 = SEAM_BYTES["thread"]
        j = np.arange(16, n, 16)
        j = j[((j // 16) % 5 == 3) & (j % PAIR_TILE != 0) & (j != n - 1) & np.isin(j // PAIR_TILE, tiles)]
        last = 0 if c["lone"] else code[SEAM_BYTES["last"]]
        p["seams"] = bool(n > 4097 and int(cnt[code[t1], code[t2]]) == sum(1 for t in tiles if t > 0)
                          and int(cnt[code[h1], code[h2]]) == j.size and j.size > 0
                          and int(cnt[code[SEAM_BYTES["first"]]].sum()) == 1 and int(cnt[:, code[SEAM_BYTES["first"]]].sum()) == 0
                          and (c["lone"] or (int(cnt[:, last].sum()) == (1 if ntiles - 1 in tiles else 0) and int(cnt[last].sum()) == 0)))
    if c["want_keys"]:
        p.update(_key_properties(c, T, exp))
    return p
