"""Small byte blocks of varied shape for sweeps over the entropy coders: alphabet size, run
structure, skew, long runs, sparse symbols, many sections."""
import numpy as np


def varied_blocks(count, max_size, seed):
    rng = np.random.default_rng(seed)
    for case in range(count):
        n = int(rng.integers(1, max_size))
        kind = case % 8
        if kind == 0:
            d = rng.integers(0, int(rng.integers(1, 257)), n)
        elif kind == 1:                                   # runs with geometric lengths
            k = max(1, n // int(rng.integers(2, 200)))
            d = np.repeat(rng.integers(0, int(rng.integers(1, 40)), k),
                          rng.geometric(1.0 / int(rng.integers(2, 400)), k))[:n]
        elif kind == 2:                                   # heavy skew
            d = np.minimum(rng.geometric(float(rng.uniform(0.05, 0.9)), n) - 1, 255)
        elif kind == 3:                                   # two symbols far apart + rare others
            d = np.where(rng.random(n) < 0.97, rng.choice([3, 250], n), rng.integers(0, 256, n))
        elif kind == 4:                                   # one very long run inside noise
            d = rng.integers(0, 6, n)
            a = int(rng.integers(0, n))
            d[a:a + int(rng.integers(1, n + 1))] = 2
        elif kind == 5:                                   # alternating pattern with defects
            d = np.arange(n) % int(rng.integers(2, 7))
            d[rng.random(n) < 0.01] = 9
        elif kind == 6:                                   # all symbols present, uniform: many sections
            d = rng.permutation(np.arange(n) % 256)
        else:                                             # power-law run lengths
            k = max(1, n // 50)
            d = np.repeat(rng.integers(0, 12, k),
                          np.minimum((rng.pareto(0.8, k) + 1).astype(np.int64), 5000))[:n]
        d = np.ascontiguousarray(d, dtype=np.uint8)
        if d.size:
            yield case, kind, d


def _synth():
    from bwtc_amd import synth
    return synth


def structured(rng, n):
    """Inputs that stress the suffix sorter: long repeats, periods, tiny alphabets, Fibonacci words."""
    kind = int(rng.integers(0, 7))
    if kind == 0:
        d = np.full(n, int(rng.integers(0, 256)))
    elif kind == 1:
        p = rng.integers(0, 256, int(rng.integers(1, 40)))
        d = np.tile(p, n // p.size + 1)[:n].copy()
        d[rng.random(n) < float(rng.uniform(0, 0.002))] = int(rng.integers(0, 256))
    elif kind == 2:
        a, b = [0], [0, 1]
        while len(b) < n:
            a, b = b, b + a
        d = np.array(b[:n]) + int(rng.integers(0, 200))
    elif kind == 3:
        d = rng.integers(0, int(rng.integers(2, 5)), n)
    elif kind == 4:
        base = rng.integers(0, 256, max(1, n // int(rng.integers(2, 50))))
        d = np.concatenate([base] * (n // base.size + 1))[:n].copy()
        k = int(rng.integers(0, 20))
        if k:
            d[rng.integers(0, n, k)] = rng.integers(0, 256, k)
    elif kind == 5:
        d = _synth().gen_text(n, int(rng.integers(1, 1 << 30)))
    else:
        d = _synth().gen_dna(n, int(rng.integers(1, 1 << 30)))
    return kind, np.ascontiguousarray(d, dtype=np.uint8)


def reference_sweep(count=400, seed=7):
    """(block, starting points) pairs on which the oracle's sorter is held to the reference's:
    small blocks of 1 to 256 symbols, every third one periodic, starting points 1 to 300.  The
    reference's answers are stored in tests/golden/bwt_ref_random.json."""
    rng = np.random.default_rng(seed)
    for it in range(count):
        n = int(rng.integers(1, 1200))
        sigma = int(rng.choice([1, 2, 3, 4, 16, 256]))
        d = rng.integers(0, sigma, n).astype(np.uint8)
        if it % 3 == 0:
            d = np.tile(d[:max(1, n // 7)], 8)[:n]
        sp = int(rng.choice([1, 2, 3, 8, 256, 300]))
        yield d, sp


def digest(a):
    """Short content digest of an array (its bytes as stored), for golden files."""
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:20]


# ---- limit cases of the entropy coders' device kernels ------------------------------------------------
# Byte strings used directly as transformed blocks (freqs = bincount, LF = [0]).  The sections follow
# from freqs alone (a section closes where the running count over symbols 0..255 reaches 10 000), so a
# deep stretch is kept inside one section by a filler symbol: a low symbol whose count is at least the
# stretch's length and whose bytes lie after it.

def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def _no_equal_neighbours(syms, counts):
    """Every symbol `counts` times, no two neighbours equal (the largest count at most half, rounded up)."""
    order = np.argsort(-np.asarray(counts, np.int64), kind="stable")
    seq = np.repeat(np.asarray(syms, np.uint8)[order], np.asarray(counts, np.int64)[order])
    half = (seq.size + 1) // 2
    assert int(np.max(counts)) <= half
    out = np.empty_like(seq)
    out[0::2] = seq[:half]
    out[1::2] = seq[half:]
    return out


def _with_filler(stretch, filler=0):
    """stretch, then `filler` bytes up to a count of at least len(stretch): section 0 is the stretch."""
    have = int(np.count_nonzero(stretch == filler))
    return np.concatenate([stretch, np.full(stretch.size - have, filler, np.uint8)])


def _fib_depth():
    # symbols 1..35 with run counts F(1)..F(35), every run one byte long: Huffman depth 34.  The runs of the
    # sixteen rarest symbols (2583 runs, codes of 19 bits and more) come first, so that the first
    # workgroups of 512 runs hold well over 8192 steps; they start with 3 1 3 2, whose codes share their
    # first 32 bits: the second and fourth run's last step lies past that common prefix (its gap flag).
    f = _fib(35)
    rare = np.concatenate([np.array([3, 1, 3, 2], np.uint8), _no_equal_neighbours(np.arange(4, 17), f[3:16])])
    rest = _no_equal_neighbours(np.arange(17, 36), f[16:])
    assert rare[4] != 2 and rare[-1] != rest[0]
    return _with_filler(np.concatenate([rare, rest]))


def _long_run_ladder(rng):
    # each section holds its own symbols: some noise of the low ones, then one long run of the highest,
    # so that the running count closes the section right after the long run
    parts, sym = [], 1
    for n in ((1 << 16) - 1, (1 << 16) + 1, (1 << 20) - 1, (1 << 20) + 1, 1 << 24, 1 << 25, 1 << 20):
        k = int(rng.integers(300, 3000))
        noise = np.repeat(rng.integers(sym, sym + 3, k).astype(np.uint8), rng.integers(1, 7, k))
        parts += [noise, np.full(n, sym + 3, np.uint8)]
        sym += 4
    return np.concatenate(parts)


def _many_long_runs(rng):
    # 74 000 runs of 512..1000 bytes over sixteen symbols (neighbours differ): 16 sections
    k = 74000
    s = np.cumsum(1 + rng.integers(0, 15, k)) % 16
    return np.repeat((s * 9 + 40).astype(np.uint8), rng.integers(512, 1001, k))


SECTION_STARTS = [3 << 12, (6 << 12) + 1, (9 << 12) - 1, (12 << 12) + 15, (15 << 12) + 16 * 100 + 15,
                  18 << 12, (21 << 12) - 1, (24 << 12) + 1, (27 << 12) + 16 * 3 + 15, 30 << 12]


def _sections_inside_runs():
    # symbols 0..9 with counts that put the section starts at SECTION_STARTS; their bytes lie after a
    # stretch of long runs of symbols 200 / 201 whose borders fall nowhere near those starts
    starts = [0] + SECTION_STARTS
    counts = np.diff(starts + [starts[-1] + 12000])
    runs = np.full(30, 5000 + 3)
    body = np.repeat(np.tile(np.array([200, 201], np.uint8), 15), runs)[:starts[-1] + 20000]
    assert body.size > starts[-1]
    low = np.repeat(np.arange(len(counts), dtype=np.uint8), counts)
    return np.concatenate([body, low])


def _many_ids():
    # one section with all 256 symbols and 1200 distinct run lengths (each three times): some 1200
    # integer nodes of 256 leaves each -- far more than 65 536 dense ids
    lens = np.tile(np.arange(1, 1201), 3)
    syms = (np.arange(lens.size) % 255 + 1).astype(np.uint8)
    syms[::97] = 0                                      # symbol 0 inside the section too (between two others)
    stretch = np.repeat(syms, lens)
    if stretch[-1] == 0:
        stretch = np.concatenate([stretch, np.array([5], np.uint8)])
    return _with_filler(stretch)


_LIMIT_CASES = [
    ("fib_depth", _fib_depth, {"max_code_len_H": 34, "max_code_len_B": 34, "max_window_steps": 8193,
                               "gap_past_32_bits": 2}),
    ("one_run_64M_minus_1", lambda: np.full((1 << 26) - 1, 77, np.uint8),
     {"max_gamma_bits": 51, "longest_run": (1 << 26) - 1}),
    ("one_run_64M", lambda: np.full(1 << 26, 77, np.uint8), {"max_gamma_bits": 53, "longest_run": 1 << 26}),
    ("one_run_64M_plus_1", lambda: np.full((1 << 26) + 1, 77, np.uint8),
     {"max_gamma_bits": 53, "longest_run": (1 << 26) + 1}),
    ("long_run_ladder", lambda: _long_run_ladder(np.random.default_rng(41)),
     {"longest_run": 1 << 25, "runs_ge_2p20": 4, "sections": 7, "max_gamma_bits": 51}),
    ("many_long_runs", lambda: _many_long_runs(np.random.default_rng(42)), {"long_runs": 70000, "sections": 8}),
    ("sections_inside_runs", _sections_inside_runs,
     {"starts_in_runs_at_tile_edge": 7, "starts_in_runs_at_row_edge": 4}),
    ("many_ids", _many_ids, {"max_section_symbols": 256, "max_section_lengths": 1200}),
]
LIMIT_CASE_NAMES = [c[0] for c in _LIMIT_CASES]


def limit_blocks(names=None):
    """(name, block, edge) for the limit cases of the 'H' and 'B' kernels (all, or those in `names`);
    edge = {measure: least value} over the measures of limit_measures(), which the case must reach."""
    for name, make, edge in _LIMIT_CASES:
        if names is None or name in names:
            yield name, np.ascontiguousarray(make(), dtype=np.uint8), edge


def section_runs(block, sections):
    """Per section: (run symbols, run lengths) -- runs end at section borders, as the coders count them."""
    out, beg = [], 0
    for n in sections:
        s = block[beg:beg + int(n)]
        cut = np.flatnonzero(s[1:] != s[:-1]) + 1
        starts = np.concatenate([[0], cut])
        out.append((s[starts], np.diff(np.concatenate([starts, [s.size]]))))
        beg += int(n)
    return out


def _gaps_past_32_bits(syms, codes):
    """Runs whose symbol code shares at least 32 leading bits with the previous run's and goes on past the
    first bit after that common prefix: steps whose gap flag needs the codes' bits beyond 32."""
    n, lens = 0, np.array([len(c) for c in codes])
    maybe = np.flatnonzero((lens[syms[:-1]] >= 32) & (lens[syms[1:]] >= 34))
    for a, b in zip(syms[maybe].tolist(), syms[maybe + 1].tolist()):
        ca, cb = codes[a], codes[b]
        common = next((i for i in range(min(len(ca), len(cb))) if ca[i] != cb[i]), min(len(ca), len(cb)))
        n += common >= 32 and len(cb) > common + 1
    return n


def limit_measures(block, oracle):
    """What the coders meet in `block`, from its bytes and the oracle's code lengths."""
    freqs = np.bincount(block, minlength=256).astype(np.uint32)
    sections = oracle.oracle_sections(freqs)
    runs = section_runs(block, sections)
    m = {"sections": int(sections.size), "max_code_len_H": 0, "max_code_len_B": 0, "longest_run": 0,
         "runs_ge_2p20": 0, "long_runs": 0, "max_window_steps": 0, "max_section_symbols": 0,
         "max_section_lengths": 0, "gap_past_32_bits": 0}
    steps = []
    for syms, lens in runs:
        rf = np.bincount(syms, minlength=256)
        ch = oracle.oracle_huffman_lengths(rf)
        cb = oracle.oracle_wavelet_code_lengths(rf)
        m["max_code_len_H"] = max(m["max_code_len_H"], int(ch.max()))
        m["max_code_len_B"] = max(m["max_code_len_B"], int(cb.max()))
        m["longest_run"] = max(m["longest_run"], int(lens.max()))
        m["runs_ge_2p20"] += int(np.count_nonzero(lens >= (1 << 20)))
        m["long_runs"] += int(np.count_nonzero(lens >= 512))
        m["max_section_symbols"] = max(m["max_section_symbols"], int(np.count_nonzero(rf)))
        m["max_section_lengths"] = max(m["max_section_lengths"], int(np.unique(lens).size))
        steps.append(cb[syms].astype(np.int64))        # symbol-tree steps of a run (its length's come on top)
        if syms.size > 1 and cb.max() > 33:
            m["gap_past_32_bits"] += _gaps_past_32_bits(syms, oracle.oracle_wavelet_codes(rf))
    steps = np.concatenate(steps)
    pad = (-steps.size) % 512                          # k_wt_expand: 512 runs per workgroup, block-wide
    m["max_window_steps"] = int(np.concatenate([steps, np.zeros(pad, np.int64)]).reshape(-1, 512).sum(1).max())
    m["max_gamma_bits"] = 2 * (m["longest_run"].bit_length() - 1) + 1
    starts = np.cumsum(sections)[:-1]
    inside = starts[block[starts] == block[starts - 1]]
    m["starts_in_runs_at_tile_edge"] = int(np.count_nonzero(np.isin(inside % 4096, (0, 1, 4095))))
    m["starts_in_runs_at_row_edge"] = int(np.count_nonzero(inside % 16 == 15))
    return m
