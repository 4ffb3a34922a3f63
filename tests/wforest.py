"""Test-side builder of flattened wavelet forests (bwtc_hip_wforest), the part tests/pgrammar.py plays for
grammars: it writes the node bit vectors the way the ENCODER fills them (every run appends one bit to each node on
its path, in run order), so what the rebuild must give back -- the runs, expanded -- is known without any decoder.
Also: the framing of wavelet streams (records of a stream) and the inputs the decoder tests share."""
import numpy as np

from bwtc_amd import hip

LINE_WORDS = 7          # the device directory's line: 7 words of bits + their prefix


# ---- codes ---------------------------------------------------------------------------------------------------
def complete_code(symbols, skew=False):
    """A complete prefix code over `symbols`: balanced, or a comb (lengths 1, 2, 3, ...) when skew."""
    symbols = list(symbols)
    if len(symbols) == 1:
        return {symbols[0]: "0"}
    if skew:
        code = {s: "1" * i + "0" for i, s in enumerate(symbols[:-1])}
        code[symbols[-1]] = "1" * (len(symbols) - 1)
        return code
    out = {}

    def split(part, prefix):
        if len(part) == 1:
            out[part[0]] = prefix
            return
        h = (len(part) + 1) // 2
        split(part[:h], prefix + "0")
        split(part[h:], prefix + "1")
    split(symbols, "")
    return out


def escape_bits(length, W):
    """The fixed code of a run length: leadingOnes ones, a zero, then leadingOnes + W bits, most significant first,
    of length - 1 - ((2^leadingOnes - 1) << W)."""
    lo = 0
    while length - 1 - (((1 << lo) - 1) << W) >= (1 << (lo + W)):
        lo += 1
    v = length - 1 - (((1 << lo) - 1) << W)
    assert 0 <= v < (1 << (lo + W))
    return "1" * lo + "0" + (format(v, "0%db" % (lo + W)) if lo + W else "")


class _Trie:
    def __init__(self):
        self.left, self.right, self.has_symbol, self.symbol, self.bits = [-1], [-1], [0], [0], [[]]

    def new(self):
        for lst, v in ((self.left, -1), (self.right, -1), (self.has_symbol, 0), (self.symbol, 0)):
            lst.append(v)
        self.bits.append([])
        return len(self.left) - 1

    def child(self, nd, bit):
        side = self.right if bit else self.left
        if side[nd] < 0:
            side[nd] = self.new()
        return side[nd]

    def add_code(self, code):
        for sym, word in code.items():
            nd = 0
            for ch in word:
                nd = self.child(nd, ch == "1")
            self.has_symbol[nd], self.symbol[nd] = 1, sym


def section(runs, W=0, sym_code=None, len_code=None, skew=False):
    """One section from its runs [(symbol, length), ...].  sym_code: {symbol: bits} (default: a complete code over the
    symbols that occur); len_code: {length: bits} with 0 = escape (None: plainFixed, every run escape coded;
    lengths without a code of their own are escape coded behind the code of 0).  Returns a dict of the section's
    tables with `node_bits` still as lists."""
    syms = sorted({s for s, _ in runs})
    sym_code = sym_code or complete_code(syms, skew)
    tree = _Trie()
    tree.add_code(sym_code)
    symbol_nodes = len(tree.left)
    codes = _Trie()
    if len_code is None:
        codes.has_symbol[0], codes.symbol[0] = 1, 0
    else:
        codes.add_code(len_code)
    reads = 0
    for s, length in runs:
        path = sym_code[s]
        if len_code is None:
            path += escape_bits(length, W)
        elif length in len_code and length != 0:
            path += len_code[length]
        else:
            path += len_code[0] + escape_bits(length, W)
        nd = 0
        for ch in path:
            tree.bits[nd].append(ch == "1")
            reads += 1
            nd = tree.child(nd, ch == "1")        # the decoder makes the node a bit goes to, also the last one's
    return dict(runs=list(runs), W=W, plain_fixed=int(len_code is None), symbol_nodes=symbol_nodes, tree=tree, codes=codes,
                reads=reads)


def pack(sections, gap_words=0):
    """Sections -> hip.Forest; every node's bits start at a word boundary (gap_words unused words between nodes).
    Returns (forest, expected bytes as a list of (symbol, length) runs, bit reads)."""
    secs, nodes, codes, words = [], [], [], []
    runs, reads = [], 0
    for sec in sections:
        t, c = sec["tree"], sec["codes"]
        secs.append((len(sec["runs"]), sum(n for _, n in sec["runs"]), len(nodes), sec["symbol_nodes"], len(t.left), len(codes),
                     len(c.left), sec["W"], sec["plain_fixed"]))
        for i in range(len(t.left)):
            bits = np.array(t.bits[i], np.uint8)
            first = len(words)
            if bits.size:
                padded = np.zeros((bits.size + 63) // 64 * 64, np.uint8)
                padded[:bits.size] = bits
                w = np.packbits(padded.reshape(-1, 64)[:, ::-1], axis=1).view(">u8").ravel()
                words.extend(int(x) for x in w)
                words.extend([0xFFFFFFFFFFFFFFFF] * gap_words)      # set bits nobody owns: the ranks must not see them
            nodes.append((t.left[i], t.right[i], t.has_symbol[i], t.symbol[i], bits.size, first if bits.size else 0))
        words.extend([0xFFFFFFFFFFFFFFFF] * sec.get("tail_words", 0))   # words no node owns, behind the section's
        for i in range(len(c.left)):
            codes.append((c.left[i], c.right[i], c.has_symbol[i], c.symbol[i]))
        runs += sec["runs"]
        reads += sec["reads"]
    f = hip.Forest(np.array(secs, hip.SECTION_DTYPE), np.array(nodes, hip.NODE_DTYPE), np.array(codes, hip.CODE_DTYPE),
                   np.array(words, np.uint64))
    return f, runs, reads


def with_words(sections, gap_words, total_words):
    """The same sections with unused all-ones words behind the last one, total_words words in all."""
    have = pack(sections, gap_words)[0].words.size
    assert have <= total_words
    return sections[:-1] + [dict(sections[-1], tail_words=total_words - have)]


def many_sections(count, seed=7):
    """count sections of one to three runs each, shapes rotated."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        runs = [(int(s), int(n)) for s, n in zip(rng.integers(0, 1 + k % 5, 1 + k % 3), rng.integers(1, 50, 1 + k % 3))]
        out.append(section(runs, W=k % 4, len_code=None if k % 2 else {1: "0", 0: "1"}))
    return out


LINE_SCAN_TILE = 4096   # lines one workgroup scans: one more line takes the scan of the line counts to three launches
WORD_COUNTS = (LINE_WORDS * LINE_SCAN_TILE - 1, LINE_WORDS * LINE_SCAN_TILE, LINE_WORDS * LINE_SCAN_TILE + 1,
               LINE_WORDS * 2 * LINE_SCAN_TILE + 1)


def expand(runs):
    return np.repeat(np.array([s for s, _ in runs], np.uint8), np.array([n for _, n in runs], np.int64))


# ---- hand-built cases ------------------------------------------------------------------------------------------
def cases():
    """name -> (sections, gap_words): the shapes the rebuild is held to."""
    rng = np.random.default_rng(31)
    out = {}
    out["single_symbol"] = ([section([(65, 1)] * 5 + [(65, 7)], W=2, len_code={1: "0", 0: "1"})], 0)
    runs256 = [(int(s), int(n)) for s, n in zip(rng.permutation(np.arange(3000) % 256), rng.integers(1, 9, 3000))]
    out["256_symbols"] = ([section(runs256, W=1, len_code={1: "00", 2: "01", 3: "10", 0: "11"})], 0)
    out["256_symbols_comb"] = ([section(runs256[:600], W=1, len_code={1: "0", 0: "1"}, skew=True)], 1)
    out["plain_fixed_W0"] = ([section([(int(s), int(n)) for s, n in zip(rng.integers(0, 5, 900), rng.integers(1, 70, 900))], W=0)], 0)
    out["plain_fixed_W15"] = ([section([(int(s), int(n)) for s, n in zip(rng.integers(0, 3, 500), rng.integers(1, 100000, 500))], W=15)], 0)
    # many leading ones: W = 0 and lengths up to 2^26
    out["deep_escapes"] = ([section([(1, 1), (2, (1 << 26) - 1), (1, 3), (3, 1 << 20), (2, 12345678), (1, 2)], W=0,
                                    len_code={1: "0", 0: "1"})], 2)
    out["runs_of_one"] = ([section([(int(s), 1) for s in rng.integers(0, 200, 5000)], W=3, len_code={1: "0", 0: "1"})], 0)
    # an empty right subtree: the code has a place for symbol 9, no run goes there
    out["empty_right_subtree"] = ([section([(4, 2), (4, 1), (4, 5)], W=1, sym_code={4: "0", 9: "1"}, len_code={1: "0", 2: "10", 0: "11"})], 0)
    # the root ends exactly on, one before and one after a word and a directory line (nodes below: every size on the way)
    for n in (63, 64, 65, 64 * LINE_WORDS - 1, 64 * LINE_WORDS, 64 * LINE_WORDS + 1, 128 * LINE_WORDS + 1):
        r = [(int(s), int(k)) for s, k in zip(rng.integers(0, 4, n), rng.integers(1, 6, n))]
        out["root_of_%d_bits" % n] = ([section(r, W=1, len_code={1: "0", 2: "10", 0: "11"})], 0)
    # several sections in one forest, different shapes, runs that cross wave and workgroup borders
    multi = []
    for k in range(5):
        n = (1, 64, 257, 1000, 4097)[k]
        r = [(int(s), int(v)) for s, v in zip(rng.integers(0, 2 + 50 * k, n), rng.integers(1, 40, n))]
        multi.append(section(r, W=k * 3, len_code=None if k % 2 else {1: "0", 3: "10", 0: "11"}))
    out["five_sections"] = (multi, 1)
    for gap in (0, 2, 3, 4, 5, 6, 7):              # with gap 1 above: a node starts in every slot of a 7-word line
        out["five_sections_gap_%d" % gap] = (multi, gap)
    # kWrMaxSections: a wave of the walk spans up to 64 sections, the verdict uses all its 256 threads
    out["256_sections"] = (many_sections(256), 0)
    # the scan of the line counts around one tile of lines
    base = out["root_of_%d_bits" % (64 * LINE_WORDS + 1)][0]
    for w in WORD_COUNTS:
        out["words_%d" % w] = (with_words(base, 0, w), 0)
    return out


def corrupt_cases():
    """name -> (forest, cap, error code): each malformed in one way."""
    base = [section([(1, 2), (2, 3), (1, 1), (3, 70), (2, 1)] * 40, W=1, len_code={1: "0", 2: "10", 0: "11"})]
    out = {}
    f, runs, _ = pack(base)
    total = sum(n for _, n in runs)
    n0 = f.nodes.copy(); n0["right"][0] = -1
    out["missing_child"] = (hip.Forest(f.sections, n0, f.codes, f.words), total, hip.E_W_CHILD)
    n1 = f.nodes.copy()
    deep = int(np.argmax((n1["bits"] > 0) & (np.arange(n1.size) > 0)))
    n1["bits"][deep] -= 1
    out["node_short_by_one_bit"] = (hip.Forest(f.sections, n1, f.codes, f.words), total, hip.E_W_BITS)
    for d in (-1, 1):
        s1 = f.sections.copy(); s1["bytes"][0] = int(s1["bytes"][0]) + d
        out["section_total_off_by_%+d" % d] = (hip.Forest(s1, f.nodes, f.codes, f.words), total + 1, hip.E_W_TOTAL)
    out["cap_short_by_one"] = (f, total - 1, hip.E_W_CAP)
    # an escape of 40 leading ones: a chain of right children full of ones
    sec = section([(5, 1)], W=0, len_code=None)
    t = sec["tree"]
    nd = [i for i in range(len(t.left)) if t.has_symbol[i]][0]
    t.bits[nd] = [True]
    for _ in range(40):
        nd = t.child(nd, True)
        t.bits[nd] = [True]
    out["escape_too_long"] = (pack([sec])[0], 1, hip.E_W_ESCAPE)
    n2 = f.nodes.copy(); n2["left"][0] = 0; n2["right"][0] = 0
    out["cycle"] = (hip.Forest(f.sections, n2, f.codes, f.words), total, hip.E_W_DEPTH)
    n3 = f.nodes.copy(); n3["left"][0] = n3.size
    out["link_outside_the_table"] = (hip.Forest(f.sections, n3, f.codes, f.words), total, hip.E_W_FOREST)
    f257, runs257, _ = pack(many_sections(257))
    out["257_sections"] = (f257, sum(n for _, n in runs257), hip.E_W_FOREST)
    return out


# ---- streams -----------------------------------------------------------------------------------------------------
def _read_packed(buf, pos):
    v, shift = 0, 0
    while True:
        b = int(buf[pos]); pos += 1
        v |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return v, pos


def records(stream):
    """Records of a wavelet stream without precompression: (coder letter, [(block size, record bytes), ...])."""
    stream = np.ascontiguousarray(stream, np.uint8)
    coder = chr(int(stream[0]))
    pos, out = 1, []
    while True:
        size, pos = _read_packed(stream, pos)
        if size == 0:
            return coder, out
        slices, pos = _read_packed(stream, pos)
        assert slices == 1 and stream[pos] == 0, "a block with a grammar"
        pos += 1
        n = int.from_bytes(stream[pos:pos + 6].tobytes(), "big")
        out.append((size, stream[pos:pos + 6 + n].copy()))
        pos += 6 + n


def decoder_inputs():
    """The inputs of tests/cpp/wavelet_decoder_test.cpp, restated."""
    rng = np.random.default_rng(777)
    out = [("abracadabra", np.frombuffer(b"abracadabra", np.uint8)), ("one_byte", np.frombuffer(b"x", np.uint8)),
           ("all_equal", np.full(30000, 65, np.uint8)), ("random", rng.integers(0, 256, 120000).astype(np.uint8)),
           ("dna", np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 90000)])]
    lens = rng.integers(1, 3001, 300)
    out.append(("long_runs", np.repeat(rng.integers(0, 6, 300).astype(np.uint8), lens)))
    out.append(("repeats", np.tile((rng.integers(0, 40, 5000) + 60).astype(np.uint8), 60)))
    out.append(("skew", np.minimum(rng.geometric(0.25, 150000) - 1, 250).astype(np.uint8)))
    return out
