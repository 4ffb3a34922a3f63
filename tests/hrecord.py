"""A test-side writer of 'H' BWT-block records from (sections, run symbols, run lengths, code lengths).

The record follows the format exactly as bwtc_hip_huffman_decode and oracle/bwtc_oracle.c decompress_H
read it: 48-bit length, n_lf - 1 and the 31-bit LF powers (flushed), the section count and the packed
section lengths, then per non-empty section the packed run count, the code shape (flushed), the
canonical Huffman codes of the run symbols (flushed) and the Elias-gamma codes of the run lengths
(flushed).  The expected transformed block of a record is np.repeat(symbols, lengths) over its sections.

Code lengths may be any prefix-free set, up to 64 bits; the oracle's Huffman lengths are used when a
section gives none.  Hooks write records damaged in one named way (see write_record's `damage`)."""
import numpy as np

TILE_BITS = 512                                        # the GPU decoder's tile (huffman_decoder.hip)


def packed(v):
    """utils::writePackedInteger: 7 bits per byte, least significant first, 0x80 = more follow."""
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def canonical_codes(clen):
    """utils::computeHuffmanCodes over 256 lengths (longest codes start at 0, a length's codes ascend
    with the symbol), as Python ints: code per symbol (0 where the length is 0)."""
    clen = [int(x) for x in clen]
    count = [0] * 65
    for L in clen:
        if L:
            count[L] += 1
    max_len = max(clen)
    first, nxt = [0] * 65, 0
    for L in range(max_len, -1, -1):
        first[L] = nxt
        nxt = (nxt + count[L]) >> 1
    code = [0] * 256
    for c in range(256):
        if clen[c]:
            code[c] = first[clen[c]]
            first[clen[c]] += 1
    return code


def kraft(clen):
    """Kraft sum of the lengths as a fraction of 2^64 (an int; 1 << 64 = complete)."""
    return sum(1 << (64 - int(L)) for L in clen if L)


def prefix_free(clen, code):
    """True when no assigned code is a prefix of another and every code fits its length."""
    cs = sorted((int(L), int(code[c])) for c, L in enumerate(clen) if L)
    if any(v >> L for L, v in cs):
        return False
    for i, (la, va) in enumerate(cs):
        for lb, vb in cs[i + 1:]:
            if (vb >> (lb - la)) == va:
                return False
    return True


def gamma_lengths(lens):
    """Bits of each run's Elias-gamma code: 2 floor(log2 len) + 1."""
    lens = np.asarray(lens)
    if lens.dtype == np.uint8:                          # short runs: a table
        return GAMMA_BITS_U8[lens]
    e = np.frexp(lens.astype(np.float64))[1].astype(np.int64)     # exact below 2^53
    return 2 * (e - 1) + 1


GAMMA_BITS_U8 = np.array([0] + [2 * (v.bit_length() - 1) + 1 for v in range(1, 256)], np.int64)


def _bits(values, widths):
    """MSB-first bit string (uint8 0/1) of `values`, each in its width."""
    n = len(values)
    if n == 0:
        return np.zeros(0, np.uint8)
    if np.ndim(widths) == 0:
        w0 = int(widths)
    else:
        widths = np.asarray(widths, np.int64)
        w0 = int(widths[0]) if (widths == widths[0]).all() else None
    if w0 is not None:                                  # one width: a 2-D unpack
        if w0 == 1:
            return (np.asarray(values) & 1).astype(np.uint8)
        if w0 == 8:
            return np.unpackbits(np.asarray(values).astype(np.uint8))
        if w0 < 8:
            return np.unpackbits(np.asarray(values).astype(np.uint8)[:, None], axis=1)[:, 8 - w0:].ravel()
        v = np.asarray(values, np.uint64)
        sh = np.arange(w0 - 1, -1, -1, dtype=np.uint64)
        return ((v[:, None] >> sh[None, :]) & np.uint64(1)).astype(np.uint8).ravel()
    v = np.asarray(values, np.uint64)
    starts = np.cumsum(widths) - widths
    out = np.zeros(int(widths.sum()), np.uint8)
    order = np.argsort(widths, kind="stable")          # codes grouped by width: work in proportion to the bits
    ws = widths[order]
    for w in np.unique(ws).tolist():
        idx = order[np.searchsorted(ws, w):np.searchsorted(ws, w, side="right")]
        vi, si = v[idx], starts[idx]
        for k in range(w):
            out[si + k] = ((vi >> np.uint64(w - 1 - k)) & np.uint64(1)).astype(np.uint8)
    return out


def _flush(bits):
    """Bytes of a bit string padded with zeros to a whole byte (HuffmanCoders.cpp flush)."""
    return np.packbits(bits)


def _bits_of(v, n):
    return [(v >> (n - 1 - i)) & 1 for i in range(n)]


def _log_ceiling(n):
    return (n - 1).bit_length() if n > 1 else 0


def _binary_code(n, lo, hi, out):
    """utils::binaryCode (Utils.hpp:239-252)."""
    rng = hi - lo + 1
    if rng == 1:
        return
    k = _log_ceiling(rng)
    short = (1 << k) - rng
    long2 = (rng - short) // 2
    if n - lo < long2:
        out += _bits_of(n - lo, k)
    elif n - lo < long2 + short:
        out += _bits_of(n - lo, k - 1)
    else:
        out += _bits_of(n - lo - short, k)


def _interpolative(lst, begin, end, lo, hi, out):
    """utils::binaryInterpolativeCode (Utils.hpp:263-281), inclusive indices."""
    if begin > end or end - begin == hi - lo:
        return
    if begin == end:
        _binary_code(lst[begin], lo, hi, out)
        return
    half = begin + (end - begin) // 2
    _binary_code(lst[half], lo + (end - begin) // 2, hi + half - end, out)
    if half > begin:
        _interpolative(lst, begin, half - 1, lo, lst[half] - 1, out)
    _interpolative(lst, half + 1, end, lst[half] + 1, hi, out)


def shape_bits(clen, max_len=None, nsym=None, deep=False):
    """HuffmanEncoder::serializeShape: max_sym, nsym (256 -> 0), packed max_len, the alphabet by
    binary interpolative coding, one unary depth per symbol.  Overrides write a damaged shape: the
    max_len and nsym fields as given, and `deep` gives the first symbol a depth of max_len + 1."""
    syms = [c for c in range(256) if clen[c]]
    true_max = max(int(clen[c]) for c in syms)
    ml = true_max if max_len is None else max_len
    ns = len(syms) if nsym is None else nsym
    out = _bits_of(syms[-1], 8) + _bits_of(ns & 0xFF, 8)
    for b in packed(ml):
        out += _bits_of(b, 8)
    _interpolative(syms, 0, len(syms) - 1, 0, syms[-1], out)
    for i, c in enumerate(syms):
        n = ml + 1 if deep and i == 0 else max(ml - int(clen[c]) + 1, 1)
        out += [0] * (n - 1) + [1]
    return np.array(out, np.uint8)


def write_record(lf, sections, damage=None, check_prefix=True):
    """One 'H' record.

    lf: the LF powers (1..256 values below 2^31).  sections: up to 256 entries (run_symbols,
    run_lengths, code_lengths or None); a section's length is the sum of its runs, an empty one has
    no body.  code_lengths: 256 lengths (0 = no code) or None for the oracle's Huffman lengths of the
    section's run symbols.  Code lengths whose canonical codes are not prefix-free are refused
    (ValueError) unless check_prefix is False.

    damage (each key optional):
      length_delta   int added to the 48-bit length field
      n_runs         {section: value} written as the run count
      max_len, nsym  {section: value} written in the shape
      deep           section whose first symbol's unary depth exceeds max_len
      section_len    {section: value} written as the section's length (the runs stay)
      h_patch        {section: {run: (value, bits)}} replaces one run's Huffman code
      cut            (part, section, bit): the record ends at the byte that holds that bit of the
                     section's part ("shape", "huffman" or "gamma")

    Returns (record bytes as uint8, facts).  facts: total, record bytes, the expected block as
    (symbols, lengths) per section, and per section S, n_runs, byte offsets of its parts and for
    each stream its exact bits, tiles (ceil(bits / 512)) and M: h_M the declared longest Huffman code,
    g_M = 2 floor(log2 S) + 1 the longest gamma code the section admits, g_longest the longest
    gamma code written."""
    import oracle_lib
    damage = damage or {}
    lf = [int(x) for x in lf]
    assert 1 <= len(lf) <= 256 and all(0 <= x < (1 << 31) for x in lf)
    assert 1 <= len(sections) <= 256
    head = _bits_of(len(lf) - 1, 8)
    for x in lf:
        head += _bits_of(x, 31)
    parts = [bytes(6), _flush(np.array(head, np.uint8)).tobytes()]
    secs, lens_field = [], []
    for i, (syms, lens, clen) in enumerate(sections):
        syms = np.asarray(syms, np.uint8)
        lens = np.asarray(lens)
        if lens.dtype != np.uint8:
            lens = lens.astype(np.uint64)
        assert syms.size == lens.size and (lens.size == 0 or lens.min() > 0)
        secs.append((syms, lens, clen))
        lens_field.append(int(damage.get("section_len", {}).get(i, int(lens.sum(dtype=np.uint64)))))
    parts.append(bytes([len(secs) & 0xFF]) + b"".join(packed(x) for x in lens_field))
    pos = sum(len(p) for p in parts)
    facts = {"sections": [], "blocks": []}
    cut_at = None
    for i, (syms, lens, clen) in enumerate(secs):
        S = int(lens.sum(dtype=np.uint64))
        facts["blocks"].append((syms, lens))
        if lens_field[i] == 0:
            facts["sections"].append({"S": 0, "n_runs": 0})
            continue
        if clen is None:
            clen = oracle_lib.oracle_huffman_lengths(np.bincount(syms, minlength=256)).astype(np.int64)
        clen = np.asarray(clen, np.int64)
        assert clen.shape == (256,) and clen.max() <= 64
        code = canonical_codes(clen)
        if check_prefix and not prefix_free(clen, code):
            raise ValueError("code lengths whose canonical codes are not prefix-free")
        used = np.flatnonzero(np.bincount(syms, minlength=256))
        assert (clen[used] > 0).all(), "a run symbol without a code"
        n_runs = int(damage.get("n_runs", {}).get(i, syms.size))
        sh = shape_bits(clen, damage.get("max_len", {}).get(i), damage.get("nsym", {}).get(i),
                        damage.get("deep") == i)
        shape = _flush(sh)
        # Huffman stream: per symbol code and length looked up by run (code values may pass 32 bits)
        cv = np.array([c & ((1 << 64) - 1) for c in code], np.uint64)
        one = np.unique(clen[used])
        hv, hl = cv[syms], (int(one[0]) if one.size == 1 else clen[syms])
        if i in damage.get("h_patch", {}):
            hl = np.broadcast_to(hl, syms.shape) if np.ndim(hl) == 0 else hl
            hv, hl = hv.copy(), hl.copy()
            for r, (v, b) in damage["h_patch"][i].items():
                hv[r], hl[r] = v, b
        hbits = _bits(hv, hl)
        if lens.dtype == np.uint8:
            gone = np.flatnonzero(np.bincount(lens, minlength=256))
            gl = GAMMA_BITS_U8[gone]
            gbits = _bits(lens, int(gl[0]) if np.unique(gl).size == 1 else GAMMA_BITS_U8[lens])
        else:
            gl = gamma_lengths(lens)
            gbits = _bits(lens, gl)
        at = {"shape": pos + len(packed(n_runs))}
        at["huffman"] = at["shape"] + shape.size
        at["gamma"] = at["huffman"] + (hbits.size + 7) // 8
        at["end"] = at["gamma"] + (gbits.size + 7) // 8
        if damage.get("cut") and damage["cut"][:2] in (("shape", i), ("huffman", i), ("gamma", i)):
            cut_at = at[damage["cut"][0]] + damage["cut"][2] // 8
        parts += [packed(n_runs), shape.tobytes(), _flush(hbits).tobytes(), _flush(gbits).tobytes()]
        pos = at["end"]
        facts["sections"].append({
            "S": S, "n_runs": int(syms.size), "at": at, "shape_bits": int(sh.size),
            "h_bits": int(hbits.size), "h_tiles": -(-int(hbits.size) // TILE_BITS), "h_M": int(clen.max()),
            "g_bits": int(gbits.size), "g_tiles": -(-int(gbits.size) // TILE_BITS),
            "g_M": 2 * (S.bit_length() - 1) + 1, "g_longest": int(gl.max())})
    rec = np.frombuffer(b"".join(parts), np.uint8).copy()
    length = rec.size - 6 + int(damage.get("length_delta", 0))
    rec[:6] = np.frombuffer(length.to_bytes(6, "big"), np.uint8)
    if cut_at is not None:
        rec = rec[:cut_at].copy()
    facts["total"] = sum(int(l.sum(dtype=np.uint64)) for _, l in facts["blocks"])
    facts["bytes"] = int(rec.size)
    facts["lf"] = lf
    return rec, facts


def expected(facts, lo=0, hi=None):
    """Bytes lo..hi of the transformed block the record stands for (np.repeat over the runs)."""
    total = facts["total"]
    hi = total if hi is None else min(hi, total)
    syms = np.concatenate([s for s, _ in facts["blocks"]] or [np.zeros(0, np.uint8)])
    lens = np.concatenate([l for _, l in facts["blocks"]] or [np.zeros(0, np.uint64)])
    if lo == 0 and hi == total:
        return np.repeat(syms, lens if lens.dtype == np.uint8 else lens.astype(np.int64))
    lens = lens.astype(np.int64)
    ends = np.cumsum(lens)
    a = int(np.searchsorted(ends, lo, side="right"))       # the run holding byte lo
    b = int(np.searchsorted(ends, hi - 1, side="right"))   # the run holding byte hi - 1
    e = ends[a:b + 1]
    ln = np.minimum(e, hi) - np.maximum(e - lens[a:b + 1], lo)
    return np.repeat(syms[a:b + 1], ln)


# ---- codes used by the tests -------------------------------------------------------------------

def fixed8():
    """A complete 8-bit code over 256 symbols."""
    return np.full(256, 8, np.int64)


def complete_code(max_len, nsym=None):
    """Complete code lengths whose longest code is max_len: symbols 0..max_len-1 get lengths
    1..max_len-1 then max_len twice (a comb).  With nsym > max_len + 1 the last level is split further
    so that nsym symbols have codes (max_len stays)."""
    clen = np.zeros(256, np.int64)
    if max_len == 1:
        clen[:2] = 1
        return clen
    clen[:max_len - 1] = np.arange(1, max_len)
    clen[max_len - 1] = clen[max_len] = max_len
    if nsym is not None:
        assert nsym <= 256
        c = max_len + 1                                 # split the shortest codes into equal halves
        while c < nsym:
            L = int(clen[:c].min())
            assert L < max_len
            s = int(np.flatnonzero(clen[:c] == L)[-1])
            clen[s] = L + 1
            clen[c] = L + 1
            c += 1
    return clen


# ---- hand-built cases --------------------------------------------------------------------------
# Each builder returns (record, facts) and each case names the edge it is built for; the tests check
# the edge from the facts (tests/test_hrecord.py) and decode the record on the GPU
# (tests/test_gpu_huffman_decode_limits.py).

CODE_SHAPE_MAX_LENS = (1, 2, 12, 13, 16, 17, 21, 22, 32, 33, 63, 64)


def _spread(syms, n, rng):
    """n run symbols: every one of `syms` at least once, the rest drawn uniformly, shuffled."""
    syms = np.asarray(syms, np.uint8)
    s = np.concatenate([syms, rng.choice(syms, max(n - syms.size, 0))])
    rng.shuffle(s)
    return s


def code_shape_case(max_len, seed=0):
    """A complete code whose longest code is max_len, every symbol used, runs of 1..5 bytes."""
    rng = np.random.default_rng(seed + max_len)
    clen = complete_code(max_len)
    syms = _spread(np.flatnonzero(clen), 3000, rng)
    return write_record([max_len], [(syms, rng.integers(1, 6, syms.size), clen)])


def incomplete_case():
    """Three 2-bit codes (00, 01, 10): prefix-free, Kraft sum 3/4."""
    rng = np.random.default_rng(3)
    clen = np.zeros(256, np.int64)
    clen[[7, 9, 200]] = 2
    syms = _spread([7, 9, 200], 5000, rng)
    return write_record([1], [(syms, rng.integers(1, 4, syms.size), clen)])


def retry_case(n_deep=6000, seed=5):
    """Section 1: a complete depth-64 code whose 64-bit codes carry almost every run, so the Huffman
    stream is far longer than a code fitted to the lengths would make it (the decoder's first,
    estimated window).  Sections 0 and 2: a fixed 8-bit code over 256 symbols, whose estimate covers
    the worst case."""
    rng = np.random.default_rng(seed)
    deep = complete_code(64)
    s1 = np.concatenate([np.arange(65), rng.choice([63, 64], n_deep)]).astype(np.uint8)
    rng.shuffle(s1)
    secs = []
    for n in (20000, None, 7000):
        if n is None:
            secs.append((s1, rng.integers(1, 9, s1.size), deep))
        else:
            secs.append((rng.integers(0, 256, n).astype(np.uint8), rng.integers(1, 9, n), fixed8()))
    return write_record([3, 9], secs)


HUFFMAN_TILE_TARGETS = (1, 63, 64, 65, 4096, 4097, 262144, 262145)


def huffman_tiles_case(n_runs):
    """A fixed 8-bit code and runs of one byte: the Huffman stream is exactly 8 n_runs bits."""
    syms = (np.arange(n_runs, dtype=np.int64) * 7 % 256).astype(np.uint8)
    return write_record([0], [(syms, np.ones(n_runs, np.uint8), fixed8())])


def huffman_tile_runs():
    """(name, n_runs, tiles): exactly T tiles, and one code short of / past the 64- and 4096-tile edges."""
    out = [("h%d" % t, 64 * t, t) for t in HUFFMAN_TILE_TARGETS]
    for t in (64, 4096):
        out += [("h%d_short" % t, 64 * t - 1, t), ("h%d_past" % t, 64 * t + 1, t + 1)]
    return out


GAMMA_TILE_TARGETS = (1, 63, 64, 65, 4096, 4097, 262144, 262145)


def gamma_tiles_case(n_runs, width):
    """One symbol (a 1-bit code) and runs of one byte (1-bit gamma codes) or of 2-3 bytes (3-bit
    gamma codes): the gamma stream is exactly width * n_runs bits."""
    clen = np.zeros(256, np.int64)
    clen[65] = 1
    if width == 1:
        lens = np.ones(n_runs, np.uint8)
    else:
        lens = (2 + (np.arange(n_runs, dtype=np.int64) * 5 % 7 < 3)).astype(np.uint8)
    return write_record([0], [(np.full(n_runs, 65, np.uint8), lens, clen)])


def gamma_tile_runs():
    """(name, n_runs, width, tiles)."""
    out = []
    for t in GAMMA_TILE_TARGETS:                       # the top level's edge: one side in each width
        if t != 262144:
            out.append(("g1_%d" % t, 512 * t, 1, t))
        if t != 262145:
            out.append(("g3_%d" % t, 512 * t // 3, 3, t))
    for t in (64, 4096):
        out += [("g1_%d_short" % t, 512 * t - 1, 1, t), ("g1_%d_past" % t, 512 * t + 1, 1, t + 1)]
    return out


def sections_cases():
    """(name, (record, facts)) of section layouts."""
    rng = np.random.default_rng(11)
    out = []
    # 256 sections (count byte 0), every third one empty
    secs = []
    for i in range(256):
        if i % 3 == 1:
            secs.append((np.zeros(0, np.uint8), np.zeros(0, np.uint64), None))
        else:
            k = int(rng.integers(1, 60))
            secs.append((rng.integers(0, 1 + i, k).astype(np.uint8), rng.integers(1, 40, k), None))
    out.append(("256_sections_with_empties", write_record([5], secs)))
    # one-byte sections
    out.append(("one_byte_sections",
                write_record([0], [(np.array([i * 37 % 256], np.uint8), np.ones(1, np.uint8), None) for i in range(200)])))
    # section borders inside runs: every section starts with the symbol the last one ended with
    secs, last = [], 4
    for i in range(40):
        k = int(rng.integers(1, 300))
        s = rng.integers(0, 6, k).astype(np.uint8)
        s[0] = last
        last = int(s[-1])
        secs.append((s, rng.integers(1, 2000, k), None))
    out.append(("borders_inside_runs", write_record([1, 2, 3], secs)))
    # 256 symbols, then 1 symbol, then 2 symbols: no table entry of one section may outlive it
    full = rng.permutation(np.concatenate([np.arange(256), rng.integers(0, 256, 5000)])).astype(np.uint8)
    out.append(("256_then_1_then_2_symbols", write_record([7], [
        (full, rng.integers(1, 4, full.size), None),
        (np.full(3, 200, np.uint8), np.array([5, 1, 9]), None),
        (np.array([0, 200, 0, 0, 200], np.uint8), np.array([1, 2, 3, 4, 5]), None)])))
    # 256 LF powers up to 2^31 - 1
    lf = [(1 << 31) - 1 - 12345 * i for i in range(256)]
    s = rng.integers(0, 256, 30000).astype(np.uint8)
    out.append(("n_lf_256", write_record(lf, [(s, rng.integers(1, 4, s.size), None)])))
    return out


# The 32-bit ceiling: run offsets in the block are 32-bit, so a block holds at most 0xFFFFFFF0 bytes.
MAX_TOTAL = 0xFFFFFFF0


def ceiling_case(total):
    """One section of `total` bytes: a 3-byte run, one of 2^31 + 1 bytes (a 63-bit gamma code), and
    the rest (near 2^32 - 2^31)."""
    lens = np.array([3, (1 << 31) + 1, total - 3 - (1 << 31) - 1], np.uint64)
    return write_record([1 << 30], [(np.array([9, 250, 17], np.uint8), lens, None)])


def damaged_cases():
    """(name, expected error name, record, oracle_checks) with the record damaged in one way.
    oracle_checks: the oracle's serial decoder checks the condition too (it must refuse)."""
    rng = np.random.default_rng(21)
    s = rng.integers(0, 40, 4000).astype(np.uint8)
    ln = rng.integers(1, 6, s.size)
    good = [(s, ln, None)]
    out = []

    def add(name, code, damage=None, sections=good, oracle=False, check_prefix=True, tail=0):
        rec, _ = write_record([2], sections, damage, check_prefix)
        if tail:
            rec = np.concatenate([rec, np.full(tail, 0x5A, np.uint8)])
        out.append((name, code, rec, oracle))

    add("max_len_0", "E_SHAPE", {"max_len": {0: 0}})
    add("max_len_65", "E_SHAPE", {"max_len": {0: 65}})
    add("nsym_above_max_sym", "E_SHAPE", {"nsym": {0: 41}})          # max_sym 39: at most 40 symbols
    add("depth_beyond_max_len", "E_SHAPE", {"deep": 0})
    over = np.zeros(256, np.int64)
    over[[3, 4, 5]] = 1                                               # Kraft sum 3/2
    add("over_full_code", "E_NO_CODE", sections=[(np.array([3, 4, 5, 3], np.uint8), np.ones(4), over)],
        check_prefix=False)
    inc = np.zeros(256, np.int64)
    inc[[7, 9, 200]] = 2                                              # 00 01 10; 11 is no code
    si = rng.choice(np.array([7, 9, 200], np.uint8), 3000)
    add("unassigned_pattern", "E_NO_CODE", {"h_patch": {0: {1700: (3, 2)}}}, sections=[(si, np.ones(si.size), inc)])
    add("n_runs_0", "E_RUNS", {"n_runs": {0: 0}})
    add("n_runs_above_section", "E_RUNS", {"n_runs": {0: int(ln.sum()) + 1}})
    # one run longer than the section: 12 bytes in a section of 10 (a 7-bit gamma code, within the
    # section's longest), and 40 bytes (an 11-bit code, past it)
    add("run_longer_than_section", "E_RUNS", {"section_len": {0: 10}},
        sections=[(np.array([4], np.uint8), np.array([12]), None)], oracle=True)
    add("run_code_longer_than_section", "E_RUNS", {"section_len": {0: 10}},
        sections=[(np.array([4], np.uint8), np.array([40]), None)], oracle=True)
    add("runs_short_of_section", "E_RUNS", {"section_len": {0: int(ln.sum()) + 3}}, oracle=True)
    # 3000 runs of 2..3 bytes where the section length says 3000 (so every run should be 1 byte): the
    # gamma stream outruns any stream of lengths that add up to the section, inside the record
    r3 = 2 + (np.arange(3000) % 2)
    add("gamma_stream_past_its_window", "E_RUNS", {"section_len": {0: 3000}},
        sections=[(np.arange(3000).astype(np.uint8), r3, None)], oracle=True)
    add("length_field_plus_1", "E_LENGTH", {"length_delta": 1}, tail=40, oracle=True)
    add("length_field_minus_1", "E_LENGTH", {"length_delta": -1}, tail=40, oracle=True)
    add("cut_in_shape", "E_PAST_RECORD", {"cut": ("shape", 0, 20)})
    add("cut_in_huffman_stream", "E_PAST_RECORD", {"cut": ("huffman", 0, 3001)})
    add("cut_in_gamma_stream", "E_PAST_RECORD", {"cut": ("gamma", 0, 2001)})
    # cut inside a gamma code's leading zeros: the bits left before the end are all zeros
    lz = np.array([1] * 7 + [1 << 20] + [1] * 10, np.uint64)       # run 7's code: 20 zeros, then 21 bits
    add("cut_in_gamma_leading_zeros", "E_PAST_RECORD", {"cut": ("gamma", 0, 16)},
        sections=[(np.arange(18).astype(np.uint8), lz, None)])
    return out
