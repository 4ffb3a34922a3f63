"""A test-side writer, reader and expansion model of `--prepr` grammars (CPU, numpy only): the counterpart of
hrecord.py for the postprocessor.  Written from the serialized format (Grammar::write / read in prepr_host.cpp,
the reference's Grammar.cpp:198-320) and from what Postprocessor::uncompress makes of it; it shares no code with
either.

The format, in order: the rule count (7 bits a byte, low group first, top bit = more); when it is not zero: the
number of special symbols and the symbols; one `large` flag per rule (first rule in the top bit); the variables
(two bytes when large: a pair of special symbols); the number of freed symbols and the symbols; the right sides'
lengths minus two (two bits each, first rule in the top bits); the right sides.

Pairs of special symbols are numbered: (i, i) -> i^2, (i, k) -> k^2 + 1 + i and (k, i) -> k^2 + k + 1 + i for i < k
(i, k: positions in the list of special symbols).  Going up the numbers, a square is the double of a special symbol
and stands for that symbol; a pair that is a large rule's variable stands for the rule; every other pair takes the
next freed symbol until none is left.  The reader learns of pairs only up to the last freed symbol or the highest
large variable, whichever is later: pairs beyond it -- doubles included -- and pairs whose second byte is not special
stand for nothing.

A symbol here is an int (a byte) or a tuple (first, second) of special bytes; a rule is (symbol, right side bytes)."""
import math

import numpy as np

KEYS = 256 + 65536


def pack_int(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def ordinal_of_pair(i, k):
    if i == k:
        return i * k
    if i > k:
        return i * (i + 1) + k + 1
    return k * k + i + 1


def pair_of_ordinal(specials, o):
    k = math.isqrt(o)
    if o == k * k:
        return (specials[k], specials[k])
    off = o - k * k - 1
    if off < k:
        return (specials[off], specials[k])
    return (specials[k], specials[off - k])


def _pair_use(specials, large_ordinals, freed):
    """What the reader knows of the pairs, by number: ("symbol", byte) or ("variable",).  None when the freed
    symbols do not fit the pairs of these special symbols."""
    ns = len(specials)
    use, left = [], list(freed)
    highest = max(large_ordinals) if large_ordinals else 0
    o = 0
    while left or (highest > 0 and o <= highest):
        k = math.isqrt(o)
        if o == k * k:
            if k >= ns:
                return None
            use.append(("symbol", specials[k]))
        elif not left or o in large_ordinals:
            use.append(("variable",))
        else:
            use.append(("symbol", left.pop(0)))
        o += 1
    return use


def _check(rules, specials, freed):
    specials, freed = list(specials), list(freed)
    assert len(rules) <= 1 << 20 and len(specials) <= 255 and len(freed) <= 255
    assert len(set(specials)) == len(specials)
    where = {z: i for i, z in enumerate(specials)}
    large = set()
    for var, rhs in rules:
        assert 2 <= len(rhs) <= 4, "a right side has 2..4 bytes"
        if isinstance(var, tuple):
            a, b = var
            assert a in where and b in where, "a large variable is a pair of special symbols"
            assert a != b, "the double of a special symbol stands for the symbol"
            large.add(ordinal_of_pair(where[a], where[b]))
        else:
            assert 0 <= var < 256 and var not in where, "a special symbol cannot be a variable"
    if rules:
        assert _pair_use(specials, large, freed) is not None, "more freed symbols than pairs to carry them"
    else:
        assert not specials and not freed, "a grammar without rules is one zero byte"
    return specials, freed, where, large


def build(rules, specials=(), freed=()):
    """The serialized grammar.  freed: original symbols in the order of the pairs they take (see the module text)."""
    specials, freed, where, _ = _check(rules, specials, freed)
    out = bytearray(pack_int(len(rules)))
    if not rules:
        return np.frombuffer(bytes(out), np.uint8)
    out.append(len(specials))
    out += bytes(specials)
    flags = bytearray((len(rules) + 7) // 8)
    for i, (var, _) in enumerate(rules):
        if isinstance(var, tuple):
            flags[i >> 3] |= 0x80 >> (i & 7)
    out += flags
    for var, _ in rules:
        out += bytes(var) if isinstance(var, tuple) else bytes([var])
    out.append(len(freed))
    out += bytes(freed)
    lens = bytearray((len(rules) + 3) // 4)
    for i, (_, rhs) in enumerate(rules):
        lens[i >> 2] |= (len(rhs) - 2) << (6 - 2 * (i & 3))
    out += lens
    for _, rhs in rules:
        out += bytes(rhs)
    return np.frombuffer(bytes(out), np.uint8)


def read(raw):
    """The inverse of build: (rules, specials, freed, bytes consumed)."""
    raw = bytes(raw) if isinstance(raw, (bytes, bytearray)) else np.ascontiguousarray(raw, np.uint8).tobytes()
    pos = count = shift = 0
    while True:
        b = raw[pos]
        pos += 1
        count |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    if count == 0:
        return [], [], [], pos
    ns = raw[pos]
    specials = list(raw[pos + 1:pos + 1 + ns])
    pos += 1 + ns
    flags = raw[pos:pos + (count + 7) // 8]
    pos += len(flags)
    variables = []
    for i in range(count):
        if flags[i >> 3] & (0x80 >> (i & 7)):
            variables.append((raw[pos], raw[pos + 1]))
            pos += 2
        else:
            variables.append(raw[pos])
            pos += 1
    nf = raw[pos]
    freed = list(raw[pos + 1:pos + 1 + nf])
    pos += 1 + nf
    lens = raw[pos:pos + (count + 3) // 4]
    pos += len(lens)
    rules = []
    for i in range(count):
        k = 2 + ((lens[i >> 2] >> (6 - 2 * (i & 3))) & 3)
        rules.append((variables[i], bytes(raw[pos:pos + k])))
        pos += k
    assert pos <= len(raw), "the grammar is cut short"
    return rules, specials, freed, pos


class Model:
    """plain[c]: what byte c stands for; paired[(a, b)]: what the pair stands for (a special; missing: nothing)."""

    def __init__(self, plain, paired, specials, n_rules, rule_bytes):
        self.plain, self.paired, self.specials, self.n_rules = plain, paired, list(specials), n_rules
        self.special = np.zeros(256, bool)
        self.special[self.specials] = True
        self.rule_bytes = rule_bytes                      # the rules' expansion lengths, in order
        self.key_len = np.zeros(KEYS, np.int64)
        self.key_src = np.zeros(KEYS, np.int64)
        pool, at = [], 0
        for key, e in [(c, plain[c]) for c in range(256)] + [(256 + (a << 8 | b), e) for (a, b), e in sorted(paired.items())]:
            self.key_len[key], self.key_src[key] = len(e), at
            pool.append(e)
            at += len(e)
        self.pool = np.frombuffer(b"".join(pool), np.uint8)
        # the keys an expansion table holds: 256 bytes and every pair that starts with a special symbol
        self.pool_bytes = int(self.key_len.sum())

    def of(self, symbol):
        return self.paired.get(symbol, b"") if isinstance(symbol, tuple) else self.plain[symbol]

    def min_cap(self):
        """The smallest capacity under which the project builds this grammar's expansions at all: no rule may stand
        for more than `cap` bytes, nor all of them together for more than 2 cap + 2^20 (prepr_host.cpp's guard
        against hostile grammars)."""
        if not self.rule_bytes:
            return 0
        return max(max(self.rule_bytes), (sum(self.rule_bytes) - (1 << 20) + 1) // 2)


def _expand_bytes(plain, paired, special, src):
    out, i = [], 0
    while i < len(src):
        if src[i] in special and i + 1 < len(src):
            out.append(paired.get((src[i], src[i + 1]), b""))
            i += 2
        else:
            out.append(plain[src[i]])
            i += 1
    return b"".join(out)


def expansions(rules, specials=(), freed=()):
    specials, freed, where, large = _check(rules, specials, freed)
    plain = [bytes([c]) for c in range(256)]
    paired = {}
    if rules:
        for o, use in enumerate(_pair_use(specials, large, freed)):
            if use[0] == "symbol":
                paired[pair_of_ordinal(specials, o)] = bytes([use[1]])
    sp = set(specials)
    sizes = []
    for var, rhs in rules:                                 # in order: a right side knows the rules before it only
        e = _expand_bytes(plain, paired, sp, bytes(rhs))
        sizes.append(len(e))
        if isinstance(var, tuple):
            paired[var] = e
        else:
            plain[var] = e
    return Model(plain, {k: v for k, v in paired.items() if v}, specials, len(rules), sizes)


def model_of(raw):
    rules, specials, freed, _ = read(raw)
    return expansions(rules, specials, freed)


def token_keys(model, data):
    """The tokens of `data` in order as table keys (a byte, or 256 + the pair), and how many of them are pairs."""
    data = np.ascontiguousarray(data, np.uint8)
    n = data.size
    if n == 0 or not model.specials:
        return data.astype(np.int32), 0
    sp = model.special[data]
    pos = np.arange(n, dtype=np.int32)
    # where the run of special bytes that ends before position i starts: behind the last byte that is not special
    run = np.maximum.accumulate(np.where(sp, 0, pos + 1).astype(np.int32))
    run[1:] = run[:-1].copy()
    run[0] = 0
    starts = ((pos - run) & 1) == 0
    del run, pos
    pair = starts & sp
    pair[n - 1] = False                                    # a special symbol that is the last byte stands alone
    keys = data.astype(np.int32)
    at = np.flatnonzero(pair)
    keys[at] = 256 + (keys[at] << 8 | data[at + 1])
    return keys[starts], int(at.size)


def token_counts(model, data):
    keys, pairs = token_keys(model, data)
    return int(keys.size), pairs


def expansion_size(model, data):
    keys, _ = token_keys(model, data)
    return int(model.key_len[keys].sum())


def expand(model, data, piece=16 << 20):
    """The expected output: every token's bytes, one after the other."""
    keys, _ = token_keys(model, data)
    if model.n_rules == 0:
        return np.ascontiguousarray(data, np.uint8).copy()
    lens, src = model.key_len[keys], model.key_src[keys]
    end = np.cumsum(lens)
    total = int(end[-1]) if end.size else 0
    out = np.empty(total, np.uint8)
    a = 0
    while a < keys.size:                                   # tokens [a, b): at most `piece` bytes, or one token
        base = int(end[a - 1]) if a else 0
        b = max(a + 1, int(np.searchsorted(end, base + piece, side="right")))
        l, size = lens[a:b], int(end[b - 1]) - base
        first = np.cumsum(l) - l
        idx = np.repeat(src[a:b] - first, l) + np.arange(size, dtype=np.int64)
        out[base:base + size] = model.pool[idx]
        a = b
    return out


def tile_sizes(model, data, tile=4096):
    """The bytes every tile of `tile` input positions stands for (a token belongs to the tile it starts in), and
    for every tile whether (tile start - start of the run of special bytes that reaches it) is odd."""
    data = np.ascontiguousarray(data, np.uint8)
    n = data.size
    sp = model.special[data]
    pos = np.arange(n, dtype=np.int64)
    run = np.maximum.accumulate(np.where(sp, 0, pos + 1))
    run = np.concatenate([[0], run[:-1]])
    starts = ((pos - run) & 1) == 0
    pair = starts & sp
    if n:
        pair[n - 1] = False
    nxt = np.concatenate([data[1:], [0]]).astype(np.int64)
    keys = np.where(pair, 256 + (data.astype(np.int64) << 8 | nxt), data)
    lens = np.where(starts, model.key_len[keys], 0)
    edges = np.arange(0, n, tile)
    return np.add.reduceat(lens, edges) if n else np.zeros(0, np.int64), ((edges - run[edges]) & 1) == 1


# ---- grammars with variables of exact lengths --------------------------------------------------------------

class Kit:
    """Composes rules so that a variable stands for exactly L bytes of content without a period.

    P(k) and Q(k) are the two Thue-Morse words of 2^k letters over two literals: P(k) = P(k-1) Q(k-1),
    Q(k) = Q(k-1) P(k-1).  The word is overlap-free, so it equals none of its own shifts over any stretch of
    three or more letters' period: a byte taken from a wrong pool offset, a wrong token or a wrong 16-byte group
    shows.  A variable of L bytes is the words P(k) or Q(k) (alternating) of L's binary digits, shortest first,
    folded into right sides of at most four bytes from the short end, so all rules together stand for little more
    than the longest ones."""

    def __init__(self, specials=(), freed=(), literals=(ord("a"), ord("b")), keep=()):
        self.specials, self.freed = list(specials), list(freed)
        self.rules = []
        taken = set(self.specials) | set(self.freed) | set(literals) | set(keep)
        self.spare = [c for c in range(255, -1, -1) if c not in taken]
        self.words = {(0, 0): literals[0], (0, 1): literals[1]}
        self.length = {}

    def fresh(self):
        assert self.spare, "no byte left for another variable"
        return self.spare.pop()

    def rule(self, var, rhs):
        self.rules.append((var, bytes(rhs)))
        return var

    def word(self, k, q):
        if (k, q) not in self.words:
            self.words[(k, q)] = self.rule(self.fresh(), [self.word(k - 1, q), self.word(k - 1, 1 - q)])
        return self.words[(k, q)]

    def variable(self, L, var=None):
        """A symbol (a fresh byte, or `var`: a byte or a pair of special symbols) that stands for exactly L >= 2 bytes."""
        assert L >= 2
        bits = [k for k in range(L.bit_length()) if L >> k & 1]
        parts = [self.word(k, i & 1) for i, k in enumerate(bits)]
        if len(parts) == 1:
            k = bits[0]
            parts = [self.word(k - 1, 0), self.word(k - 1, 1)]
        while len(parts) > 4:
            parts = [self.rule(self.fresh(), parts[:4])] + parts[4:]
        var = self.rule(self.fresh() if var is None else var, parts)
        self.length[var] = L
        return var

    def grammar(self):
        return build(self.rules, self.specials, self.freed)

    def model(self):
        m = expansions(self.rules, self.specials, self.freed)
        for var, L in self.length.items():
            assert len(m.of(var)) == L, (var, L, len(m.of(var)))
        return m


def symbols(seq):
    """Input bytes from a sequence of symbols (bytes and pairs)."""
    out = bytearray()
    for s in seq:
        out += bytes(s) if isinstance(s, tuple) else bytes([s])
    return np.frombuffer(bytes(out), np.uint8)


# ---- the hand-built grammars of the limits tests ---------------------------------------------------------------

TOKEN_LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 255, 4095, 4096, 4097, 65535, 65537, (1 << 20) + 1)
PLAIN = (ord("x"), ord("y"), ord("z"))                     # bytes no grammar here gives a rule


def length_grammar(L):
    """(kit, variable of L bytes, variables of the other lengths up to L that take part in the mixes).  L = 1 is
    a byte without a rule."""
    kit = Kit(keep=PLAIN)
    others = {}
    for m in TOKEN_LENGTHS:
        if 2 <= m <= max(L, 33) and m != L and (m <= 4097 or m == L):
            others[m] = kit.variable(m)
    var = PLAIN[0] if L == 1 else kit.variable(L)
    return kit, var, others


SPECIALS = tuple(range(0xE0, 0xF0))                        # sixteen special symbols: pair numbers up to 255
FREED = (0x01, 0x02, 0x03, 0x04, 0x05)
LARGE = (((0xE1, 0xE0), 5), ((0xE3, 0xE7), 17), ((0xEF, 0xEE), 33), ((0xEF, 0xE0), 4097), ((0xE2, 0xEF), 2))
EMPTY_PAIR = (0xE9, 0xEA)                                  # nobody defines it: it stands for nothing


def special_kit():
    """Sixteen special symbols, five freed symbols, large variables of 2, 5, 17, 33 and 4097 bytes (the highest is
    pair number 255), byte variables of 3, 16 and 255 bytes; the other pairs stand for nothing."""
    kit = Kit(specials=SPECIALS, freed=FREED, keep=PLAIN)
    for m in (3, 16, 255):
        kit.variable(m)
    for pair, m in LARGE:
        kit.variable(m, pair)
    return kit


def two_special_kit():
    """The issue's second hand-written shape: two special symbols, one large variable, one freed symbol."""
    kit = Kit(specials=(0xF0, 0xF1), freed=(0x07,), keep=PLAIN)
    kit.variable(9, (0xF1, 0xF0))
    kit.variable(6)
    return kit


def small_grammars():
    """name -> kit: every hand-built grammar shape the GPU limits file uses."""
    out = {"special16": special_kit(), "special2": two_special_kit()}
    for L in TOKEN_LENGTHS:
        out["length_%d" % L] = length_grammar(L)[0]
    return out


def mix(rng, alphabet, n, weights=None):
    """n symbols drawn from `alphabet` (bytes and pairs) as input bytes."""
    pick = rng.choice(len(alphabet), size=n, p=weights)
    return symbols(alphabet[int(i)] for i in pick)


def long_mix(rng, short, var, L, n=300, budget=16 << 20):
    """n symbols of `short` with copies of `var` (L bytes each) among them: several hundred tokens whose boundaries
    fall anywhere in a 16-byte group; as many of the long token as `budget` output bytes allow (3..100)."""
    seq = [short[int(i)] for i in rng.integers(0, len(short), n)]
    for at in sorted(rng.integers(0, n, min(100, max(3, budget // L))).tolist(), reverse=True):
        seq.insert(at, var)
    return symbols(seq)
