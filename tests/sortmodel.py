"""Test-side model of the radix sorts (bwtc_amd/csrc/radix_sort.hpp), the part tests/invmodel.py plays for the inverse
transform: plain numpy, nothing of bwtc_amd.

Three forms, as the hooks bwtc_hip_test_radix_* expose them:
  plain      radix_sort_pairs: stable by the bits the passes really cover -- whole 8-bit digits from bit_lo, so the
             covered field is [bit_lo, bit_lo + 8 * passes), passes = ceil((nbits - bit_lo) / 8) (with holes at least
             one: the compacting pass).  Holes (all-ones keys) are removed first.  Everything outside the covered field
             is payload: it comes back attached to its item and never moves one.
  long       radix_sort_long: stable by ((key & (2^kbits - 1)) << wbits) | w; key bits at and above kbits are payload.
             long_plan() restates the pass plan: w's whole digits, the bridge digit with r bits of w, the key's digits.
  segmented  radix_sort_keys_segmented: every segment (whole tiles) stably sorted on its own by bits
             [bit_lo, bit_lo + 16); the all-ones padding has the largest field and stays at its segment's end.
cases() lists the named cases tests/test_gpu_sort_limits.py runs, each a small dict with a fixed seed; make() draws a
case's input, expected() is the model's answer, properties() says from the drawn input which edges the case reaches
(tests/test_sortmodel.py holds every case to the edges it is named for)."""
import numpy as np

RADIX_BITS = 8
TPB = 512                                       # kRadixTPB
TILE = {"u32": 16 * TPB, "u64": 8 * TPB}        # radix_tile<K>()
LONG_TILE = {6: 6 * TPB, 8: 8 * TPB}            # kRadixTPB * EL
LONG_INSTS = (("u32", 6), ("u16", 6), ("u16", 8))   # (V, EL) the suffix sorter instantiates
SCAN_TILE = 4096                                # kScanTile: an offset table of more words takes the three-launch scan
STEP_LEAF_SHIFT = 2                             # kStepLeafShift: where the step sort's field starts
DT = {"u16": np.uint16, "u32": np.uint32, "u64": np.uint64}
WIDTH = {"u32": 32, "u64": 64}
U64 = np.uint64


def _mask(bits):
    return U64((1 << bits) - 1) if bits < 64 else U64(0xFFFFFFFFFFFFFFFF)


def _ones(dtype):
    return np.dtype(dtype).type(np.iinfo(dtype).max)


def _shr(a, s):
    a = np.asarray(a).astype(U64)
    return a >> U64(s) if s < 64 else np.zeros_like(a)


def _shl(a, s):
    a = np.asarray(a).astype(U64)
    return a << U64(s) if s < 64 else np.zeros_like(a)


def _bits(rng, n, bits):
    """n random numbers of `bits` bits (uint64)."""
    if bits <= 0:
        return np.zeros(n, U64)
    return rng.integers(0, 1 << bits, n, dtype=U64)


# ---- the plain sort ------------------------------------------------------------------------------------------------
def passes(bit_lo, nbits, holes=False):
    p = -(-(nbits - bit_lo) // RADIX_BITS)
    return max(p, 1) if holes else p


def boundary(bit_lo, nbits, width, holes=False):
    """End of the field the passes cover (cut to the key's width)."""
    return min(width, bit_lo + RADIX_BITS * passes(bit_lo, nbits, holes))


def field(keys, bit_lo, nbits, holes=False):
    width = 8 * np.asarray(keys).dtype.itemsize
    return _shr(keys, bit_lo) & _mask(boundary(bit_lo, nbits, width, holes) - bit_lo)


def digit(keys, shift):
    """radix_digit(key, shift)."""
    return (_shr(keys, shift) & U64(255)).astype(np.int64)


def plain_expected(keys, vals=None, n_holes=0, bit_lo=0, nbits=None, values="given", vtype="u32"):
    """-> (sorted keys, their values or None)."""
    keys = np.asarray(keys)
    nbits = 8 * keys.itemsize if nbits is None else nbits
    live = np.flatnonzero(keys != _ones(keys.dtype)) if n_holes else np.arange(keys.size)
    n = live.size
    assert n == keys.size - n_holes, "the all-ones keys are the holes"
    if n > 1 or n_holes:
        order = np.argsort(field(keys[live], bit_lo, nbits, n_holes > 0), kind="stable")
    else:
        order = np.arange(n)                    # no pass is made
    src = live[order]                           # the slot every output item came from
    if values == "keys":
        out_v = None
    elif values == "given":
        out_v = np.asarray(vals)[src].astype(DT[vtype])
    else:
        assert n_holes == 0 and n >= 2 and nbits > bit_lo, "the first pass makes the values up"
        out_v = (src if values == "positions" else n - 1 - src).astype(np.uint32).astype(DT[vtype])
    return keys[src], out_v


# ---- the long sort -------------------------------------------------------------------------------------------------
def long_plan(kbits, wbits):
    """radix_sort_long's passes, first to last: dicts {src: "w" | "bridge" | "key", shift, bits, r}.  A bridge digit is
    w's top r bits (from `shift`) under the key's lowest bits - r ones; `bits` cuts a field's top digit."""
    plan, s = [], 0
    while s + RADIX_BITS <= wbits:
        plan.append(dict(src="w", shift=s, bits=RADIX_BITS, r=0))
        s += RADIX_BITS
    ks = 0
    if s < wbits:
        r = wbits - s
        plan.append(dict(src="bridge", shift=s, bits=min(RADIX_BITS, r + kbits), r=r))
        ks = min(kbits, RADIX_BITS - r)
    while ks < kbits:
        plan.append(dict(src="key", shift=ks, bits=min(RADIX_BITS, kbits - ks), r=0))
        ks += RADIX_BITS
    return plan


def long_digit(p, keys, w):
    """long_digit<K, LONG>() of pass p."""
    w64 = np.asarray(w).astype(U64)
    if p["src"] == "w":
        d = _shr(w64, p["shift"])
    elif p["src"] == "bridge":
        d = _shr(w64, p["shift"]) | (_shl(keys, p["r"]) & U64(0xFFFFFFFF))
    else:
        d = _shr(keys, p["shift"])
    return (d & _mask(p["bits"])).astype(np.int64)


def long_order(keys, w, kbits, wbits):
    return np.lexsort((np.asarray(w).astype(U64) & _mask(wbits), np.asarray(keys).astype(U64) & _mask(kbits)))


def long_order_by_passes(keys, w, kbits, wbits):
    """The same order the way the kernels reach it: one stable pass per digit of the plan."""
    order = np.arange(len(keys))
    for p in long_plan(kbits, wbits):
        order = order[np.argsort(long_digit(p, keys[order], w[order]), kind="stable")]
    return order


def long_expected(keys, w, kbits, wbits, vtype="u32"):
    """-> (keys, values, w): the values are n - 1 - (the item's input place), cut to vtype."""
    order = long_order(keys, w, kbits, wbits)
    n = len(keys)
    return keys[order], (n - 1 - order).astype(np.uint32).astype(DT[vtype]), w[order]


# ---- the segmented sort --------------------------------------------------------------------------------------------
def seg_expected(keys, bit_lo, tile_first):
    out = np.array(keys, np.uint32, copy=True)
    t = TILE["u32"]
    for s in range(len(tile_first) - 1):
        a, b = int(tile_first[s]) * t, int(tile_first[s + 1]) * t
        seg = out[a:b]
        out[a:b] = seg[np.argsort((seg >> np.uint32(bit_lo)) & np.uint32(0xFFFF), kind="stable")]
    return out


# ---- named cases ---------------------------------------------------------------------------------------------------
SEAM_TILES = (1, 2, 7, 8, 9, 16, 17)
SEAM_SMALL = (1, 2, 63, 64, 65)
SEAM_NBITS = {"u32": (1, 7, 8, 9, 16, 32), "u64": (13, 40, 56, 57, 64)}
SHAPES = ("same", "alternate", "ends", "uniform", "hot", "allones")
LONG_BITS = ((40, 32), (33, 21), (17, 7), (9, 4), (3, 4), (1, 1), (64, 32), (48, 16))
LONG_TILES = (1, 2, 9, 17)


def _plain(group, bucket, ktype, n, **kw):
    c = dict(form="plain", group=group, bucket=bucket, ktype=ktype, vtype="u32", n=n, n_holes=0, layout=None, bit_lo=0,
             nbits=WIDTH[ktype], values="given", planes=0, shape="random", payload=False, few=0, edge={})
    c.update(kw)
    c["name"] = "plain-%s-%s-%s-n%d-h%d%s-b%d_%d-%s-p%d-%s%s%s" % (
        group, ktype, c["vtype"], n, c["n_holes"], "-" + c["layout"] if c["layout"] else "", c["bit_lo"], c["nbits"], c["values"],
        c["planes"], c["shape"], "-payload" if c["payload"] else "", "-few%d" % c["few"] if c["few"] else "")
    return c


def _seam_edge(n, tile):
    tiles = -(-n // tile)
    return dict(tiles=tiles, rem=n % tile, scan_tiles=-(-tiles * 256 // SCAN_TILE), unused_slots=-(-tiles // 8) * 8 - tiles,
                odd_pair=tiles % 2)


def _plain_cases():
    out = []
    for ktype in ("u32", "u64"):
        T = TILE[ktype]
        sizes = list(SEAM_SMALL) + [t * T + d for t in SEAM_TILES for d in (-1, 0, 1)]
        for n in sizes:
            for planes in (0, 1):
                for nbits in SEAM_NBITS[ktype]:
                    out.append(_plain("seams", "%s-n%d" % (ktype, n), ktype, n, nbits=nbits, planes=planes, edge=_seam_edge(n, T)))
        two = (T + 1, 9 * T - 1)
        for shape in SHAPES:
            for n in two:
                for planes in (0, 1):
                    out.append(_plain("digits", "%s-%s" % (ktype, shape), ktype, n, shape=shape, planes=planes,
                                      edge=dict(shape_ok=True, tiles=-(-n // T))))
        # payload beside the sorted field
        if ktype == "u64":
            for nbits in (40, 48, 56):
                for n in two:
                    for planes in (0, 1):
                        out.append(_plain("payload", "u64-bits56_63", ktype, n, nbits=nbits, planes=planes, payload=True, few=37,
                                          edge=dict(high_varies=True, top8_varies=True, has_ties=True)))
        lows = {"u32": ((8, 32), (12, 28), (12, 32)), "u64": ((8, 40), (12, 33), (32, 49), (40, 64), (36, 52))}[ktype]
        for bit_lo, nbits in lows:
            for n in two:
                for planes in (0, 1, 2):
                    out.append(_plain("payload", "%s-bit_lo%d" % (ktype, bit_lo), ktype, n, bit_lo=bit_lo, nbits=nbits, planes=planes,
                                      payload=True, few=1021, edge=dict(low_varies=True, has_ties=True)))
        # values the first pass makes up, keys only, 16-bit values
        vn = [t * T + d for t in (1, 2, 9) for d in (-1, 1)]
        nb = {"u32": 20, "u64": 48}[ktype]
        for values, vtype in (("positions", "u32"), ("descending", "u32"), ("keys", "u32"), ("given", "u16"), ("descending", "u16")):
            for n in vn:
                for planes in (0, 2):
                    kw = dict(values=values, vtype=vtype, nbits=nb, planes=planes, edge=dict(tiles=-(-n // T), top_digit_bits=nb % 8 or 8))
                    if values == "keys" and ktype == "u32":       # the step sort's shape: field from kStepLeafShift, plane ready
                        kw.update(bit_lo=STEP_LEAF_SHIFT, nbits=19, payload=True, edge=dict(tiles=-(-n // T), low_varies=True))
                    out.append(_plain("values", "%s-%s-%s" % (ktype, values, vtype), ktype, n, **kw))
        # holes
        hb = {"u32": 24, "u64": 40}[ktype]
        hn = (T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 9 * T - 1, 9 * T + 1)
        for n in hn:
            for planes in (0, 1):
                lay = [(1, "end"), (1, "random"), (T - 1, "one_tile"), (T - 1, "end"), (T, "whole_tile"), (T, "end"), (n, "alternate"),
                       (n, "end")]
                for h, layout in sorted(set(lay), key=lay.index):
                    edge = dict(first_tiles=-(-(n + h) // T))
                    if layout == "one_tile":
                        edge.update(hole_tiles=1, full_hole_tiles=0)
                    if layout == "whole_tile":
                        edge.update(hole_tiles=1, full_hole_tiles=1)
                    if layout == "end":
                        edge.update(holes_at_end=True)
                    if layout == "alternate":
                        edge.update(holes_alternate=True)
                    out.append(_plain("holes", "%s-n%d" % (ktype, n), ktype, n, n_holes=h, layout=layout, nbits=hb, planes=planes,
                                      payload=True, edge=edge))
        for planes in (0, 1):
            for h, layout in ((1, "end"), (T, "random"), (3, "random")):
                out.append(_plain("holes", "%s-n1" % ktype, ktype, 1, n_holes=h, layout=layout, nbits=hb, planes=planes, payload=True,
                                  edge=dict(first_tiles=-(-(1 + h) // T))))
            for n in two:
                for h, layout in ((T - 1, "random"), (n, "alternate")):
                    out.append(_plain("holes", "%s-nbits0" % ktype, ktype, n, n_holes=h, layout=layout, nbits=0, planes=planes, payload=True,
                                      edge=dict(passes=1, order_kept=True)))
    return out


def _long_cases():
    out = []
    for vtype, el in LONG_INSTS:
        T = LONG_TILE[el]
        for t in LONG_TILES:
            for d in (-1, 1):
                n = t * T + d
                for direct in (1, 0):
                    for kbits, wbits in LONG_BITS:
                        out.append(_long(vtype, el, n, kbits, wbits, direct, 0))
        for direct in (1, 0):
            for kbits, wbits in LONG_BITS:
                out.append(_long(vtype, el, 9 * T + 1, kbits, wbits, direct, 3))
    return out


def _long(vtype, el, n, kbits, wbits, direct, few):
    T = LONG_TILE[el]
    plan = long_plan(kbits, wbits)
    r = wbits % 8
    edge = dict(tiles=-(-n // T), passes=-(-(kbits + wbits) // 8), bridge_r=r, first_is_bridge=wbits < 8,
                single_masked_digit=wbits < 8 and r + kbits < 8, payload_bits=64 - kbits, payload_varies=kbits < 64)
    if few:
        edge["ties_span_tiles"] = True
    assert len(plan) == edge["passes"]
    return dict(form="long", group="long", bucket="%s-e%d-n%d%s" % (vtype, el, n, "-few" if few else ""), vtype=vtype, el=el, n=n, kbits=kbits,
                wbits=wbits, direct_w=direct, few=few, edge=edge,
                name="long-%s-e%d-n%d-k%d-w%d-%s%s" % (vtype, el, n, kbits, wbits, "words" if direct else "planes", "-few%d" % few if few else ""))


def _seg(label, seg_tiles, bit_lo, fill="random", edge=None):
    e = dict(nseg=len(seg_tiles), tiles=sum(seg_tiles))
    e.update(edge or {})
    return dict(form="seg", group="seg", bucket=label, seg_tiles=tuple(seg_tiles), bit_lo=bit_lo, fill=fill, edge=e,
                name="seg-%s-b%d-%s" % (label, bit_lo, fill))


def _seg_cases():
    out = []
    many = [0] * 256                             # 256 segments, most of them empty: empties first, in a row, in the middle, last
    for s, t in ((3, 1), (4, 2), (5, 0), (6, 0), (7, 9), (100, 1), (101, 1), (200, 2), (250, 1)):
        many[s] = t
    full = [1, 2, 1] * 85 + [9]                  # 256 segments, none empty
    for bit_lo in (0, STEP_LEAF_SHIFT):
        for t in (1, 2, 9):
            out.append(_seg("one_segment_%d" % t, [t], bit_lo))
        out.append(_seg("two_segments", [1, 2], bit_lo))
        out.append(_seg("two_segments_9_1", [9, 1], bit_lo))
        out.append(_seg("empty_first", [0, 2], bit_lo, edge=dict(empty_first=True)))
        out.append(_seg("empty_last", [2, 0], bit_lo, edge=dict(empty_last=True)))
        out.append(_seg("many_empty", many, bit_lo, edge=dict(empty_first=True, empty_last=True, empty_middle=True, empty_run=True)))
        out.append(_seg("all_256", full, bit_lo))
        out.append(_seg("lonely_key", [1, 2, 0, 1], bit_lo, fill="lonely", edge=dict(lonely=True, empty_middle=True)))
        out.append(_seg("max_field", [1, 2, 9], bit_lo, fill="max_field", edge=dict(max_field_next_to_padding=True)))
    return out


_CASES = None


def cases(group=None):
    global _CASES
    if _CASES is None:
        _CASES = _plain_cases() + _long_cases() + _seg_cases()
        for i, c in enumerate(_CASES):
            c["seed"] = 7919 * i + 17
        assert len({c["name"] for c in _CASES}) == len(_CASES)
    return [c for c in _CASES if group is None or c["group"] == group]


def buckets(group):
    seen = []
    for c in cases(group):
        if c["bucket"] not in seen:
            seen.append(c["bucket"])
    return seen


# ---- a case's input ------------------------------------------------------------------------------------------------
def _shape_field(shape, n, F, few, rng):
    i = np.arange(n, dtype=U64)
    npass = -(-F // 8)
    if few:
        f = _bits(rng, few, F)[rng.integers(0, few, n)]
    elif shape in ("random", "allones"):
        f = _bits(rng, n, F)
    elif shape == "same":
        f = np.full(n, _bits(rng, 1, F)[0], U64)
    elif shape == "alternate":
        f = np.where(i % U64(2) == 0, U64(0x1111111111111111), U64(0xEEEEEEEEEEEEEEEE))
    elif shape == "ends":
        f = np.zeros(n, U64)
        for j in range(npass):
            f |= _shl(rng.integers(0, 2, n).astype(U64) * U64(255), 8 * j)
    elif shape == "uniform":
        f = np.zeros(n, U64)
        for j in range(npass):
            m, o = U64(2 * int(rng.integers(0, 128)) + 1), U64(int(rng.integers(0, 256)))
            f |= _shl((i * m + o) % U64(256), 8 * j)
    elif shape == "hot":
        f = np.full(n, _bits(rng, 1, F)[0], U64)
        cold = rng.permutation(n)[:max(1, n // 100)]
        f[cold] = _bits(rng, cold.size, F)
    else:
        raise ValueError(shape)
    return f & _mask(F)


def _hole_mask(layout, n, h, T, rng):
    n_in = n + h
    m = np.zeros(n_in, bool)
    if layout == "end":
        m[n:] = True
    elif layout == "random":
        m[rng.permutation(n_in)[:h]] = True
    elif layout in ("one_tile", "whole_tile"):
        t0 = 1 if n_in >= 2 * T else 0
        a = t0 * T + (T - h + 1) // 2               # TILE - 1 holes: slots 1 .. TILE - 1 of the tile
        m[a:a + h] = True
    elif layout == "alternate":
        m[1:2 * h:2] = True
    else:
        raise ValueError(layout)
    assert int(m.sum()) == h
    return m


def make(c):
    """The case's input: a dict of arrays (the same every time)."""
    rng = np.random.default_rng(c["seed"])
    if c["form"] == "plain":
        W, n, h = WIDTH[c["ktype"]], c["n"], c["n_holes"]
        bit_lo, nbits = c["bit_lo"], c["nbits"]
        end = boundary(bit_lo, nbits, W, h > 0)
        k = _shl(_shape_field(c["shape"], n, nbits - bit_lo, c["few"], rng), bit_lo)      # bits [nbits, end) stay zero
        if c["payload"]:
            k |= _bits(rng, n, bit_lo) | _shl(_bits(rng, n, W - end), end)
        if c["shape"] == "allones":
            k[rng.permutation(n)[:max(1, n // 20)]] = _mask(W)
        k = k.astype(DT[c["ktype"]])
        if h:
            assert not (k == _ones(k.dtype)).any()
            full = np.full(n + h, _ones(k.dtype), k.dtype)
            full[~_hole_mask(c["layout"], n, h, TILE[c["ktype"]], rng)] = k
            k = full
        inp = dict(keys=k)
        if c["values"] == "given":
            inp["vals"] = _bits(rng, n + h, 8 * np.dtype(DT[c["vtype"]]).itemsize).astype(DT[c["vtype"]])
        return inp
    if c["form"] == "long":
        n, kbits, wbits = c["n"], c["kbits"], c["wbits"]
        if c["few"]:
            pick = rng.integers(0, c["few"], n)
            k, w = _bits(rng, c["few"], kbits)[pick], _bits(rng, c["few"], wbits)[rng.integers(0, c["few"], n)]
        else:
            # few enough values for equal (key, w) items to exist, spread over every digit: 2^10 of each word
            k = _bits(rng, n, min(kbits, 10)) * U64(0x9E3779B97F4A7C15) & _mask(kbits)
            w = _bits(rng, n, min(wbits, 10)) * U64(0x9E3779B97F4A7C15) & _mask(wbits)
        k |= _shl(_bits(rng, n, 64 - kbits), kbits)                                       # payload above kbits
        return dict(keys=k, w=w.astype(np.uint32))
    T = TILE["u32"]
    tf = np.concatenate([[0], np.cumsum(c["seg_tiles"])]).astype(np.uint32)
    bit_lo = c["bit_lo"]
    k = np.empty(int(tf[-1]) * T, np.uint32)
    for s, t in enumerate(c["seg_tiles"]):
        if t == 0:
            continue
        a, m = int(tf[s]) * T, t * T
        real = 1 if c["fill"] == "lonely" and s == 0 else int(rng.integers(max(1, m - T + 1), m + 1))   # padding only in the last tile
        if c["fill"] == "lonely" and s == 1:
            real = m                                 # and a segment without padding beside it
        f = rng.integers(0, 1 << 16, real, dtype=np.uint32)
        pay = rng.integers(0, 1 << 32, real, dtype=np.uint64).astype(np.uint32) & ~np.uint32(0xFFFF << bit_lo)
        if c["fill"] == "max_field":
            top = rng.permutation(real)[:max(2, real // 8)]
            f[top] = 0xFFFF
            f[real - 1] = 0xFFFF                     # the last real key sits right before the padding
            pay[top] &= ~np.uint32(1 << 31)          # never the padding's own word
            pay[real - 1] &= ~np.uint32(1 << 31)
        seg = np.full(m, 0xFFFFFFFF, np.uint32)
        seg[:real] = (f << np.uint32(bit_lo)) | pay
        k[a:a + m] = seg
    return dict(keys=k, tile_first=tf)


def expected(c, inp):
    if c["form"] == "plain":
        return plain_expected(inp["keys"], inp.get("vals"), c["n_holes"], c["bit_lo"], c["nbits"], c["values"], c["vtype"])
    if c["form"] == "long":
        return long_expected(inp["keys"], inp["w"], c["kbits"], c["wbits"], c["vtype"])
    return seg_expected(inp["keys"], c["bit_lo"], inp["tile_first"])


# ---- what a drawn input reaches ------------------------------------------------------------------------------------
def _shape_ok(c, live):
    """Does every pass see the digit shape the case is named for?  (digits as the kernels take them)"""
    n = live.size
    for p in range(passes(c["bit_lo"], c["nbits"])):
        d = digit(live, c["bit_lo"] + 8 * p)
        cnt = np.bincount(d, minlength=256)
        if c["shape"] == "same":
            ok = int((cnt > 0).sum()) == 1
        elif c["shape"] == "alternate":
            ok = int((cnt > 0).sum()) == 2 and (d[0::2] == d[0]).all() and (d[1::2] == d[1]).all() and d[0] != d[1]
        elif c["shape"] == "ends":
            ok = cnt[0] > 0 and cnt[255] > 0 and cnt[0] + cnt[255] == n
        elif c["shape"] == "uniform":
            ok = int(cnt.min()) == n // 256 and int(cnt.max()) <= n // 256 + 1
        elif c["shape"] == "hot":
            ok = int(cnt.max()) * 100 >= 99 * n and int((cnt > 0).sum()) > 1
        elif c["shape"] == "allones":
            ok = True
        else:
            return None
        if not ok:
            return False
    if c["shape"] == "allones":
        return bool((live == _ones(live.dtype)).any()) and c["n_holes"] == 0 and c["nbits"] == WIDTH[c["ktype"]]
    return True


def properties(c, inp):
    """Edges the drawn input reaches, by name (see the `edge` dict of every case)."""
    k = inp["keys"]
    if c["form"] == "plain":
        T, W = TILE[c["ktype"]], WIDTH[c["ktype"]]
        h = c["n_holes"]
        hole = (k == _ones(k.dtype)) if h else np.zeros(k.size, bool)
        live = k[~hole]
        tiles = -(-k.size // T)
        end = boundary(c["bit_lo"], c["nbits"], W, h > 0)
        f = field(live, c["bit_lo"], c["nbits"], h > 0)
        per_tile = np.add.reduceat(hole.astype(np.int64), np.arange(0, k.size, T)) if k.size else np.zeros(0, np.int64)
        tile_items = np.minimum(T, k.size - np.arange(tiles) * T)
        np_ = passes(c["bit_lo"], c["nbits"], h > 0)
        return dict(tiles=-(-live.size // T), first_tiles=tiles, rem=k.size % T, scan_tiles=-(-tiles * 256 // SCAN_TILE),
                    unused_slots=-(-tiles // 8) * 8 - tiles, odd_pair=tiles % 2, passes=np_,
                    top_digit_bits=(c["nbits"] - c["bit_lo"]) - 8 * (np_ - 1),
                    shape_ok=_shape_ok(c, live),
                    low_varies=c["bit_lo"] > 0 and np.unique(live.astype(U64) & _mask(c["bit_lo"])).size > 1,
                    high_varies=end < W and np.unique(_shr(live, end)).size > 1,
                    top8_varies=W == 64 and end <= 56 and np.unique(_shr(live, 56)).size > 1,
                    has_ties=np.unique(f).size < f.size,
                    hole_tiles=int((per_tile > 0).sum()), full_hole_tiles=int((per_tile == tile_items).sum()),
                    holes_at_end=h > 0 and bool(hole[k.size - h:].all()),
                    holes_alternate=h > 0 and bool(hole[1:2 * h:2].all()) and not hole[0:2 * h:2].any(),
                    order_kept=np.unique(f).size <= 1)
    if c["form"] == "long":
        T = LONG_TILE[c["el"]]
        plan = long_plan(c["kbits"], c["wbits"])
        bridge = [p for p in plan if p["src"] == "bridge"]
        comp = np.stack([k & _mask(c["kbits"]), inp["w"].astype(U64)])
        groups = np.unique(comp, axis=1, return_counts=True)[1]
        return dict(tiles=-(-k.size // T), passes=len(plan), bridge_r=bridge[0]["r"] if bridge else 0,
                    first_is_bridge=plan[0]["src"] == "bridge",
                    single_masked_digit=len(plan) == 1 and plan[0]["src"] == "bridge" and plan[0]["bits"] < 8,
                    payload_bits=64 - c["kbits"], payload_varies=c["kbits"] < 64 and np.unique(_shr(k, c["kbits"])).size > 1,
                    has_ties=int(groups.max()) > 1, ties_span_tiles=int(groups.max()) > T,
                    words_hist_passes=sum(1 for i, p in enumerate(plan) if c["direct_w"] and i > 0 and p["src"] == "w"),
                    w_fits=c["wbits"] == 32 or not (inp["w"] >> np.uint32(c["wbits"])).any())
    T = TILE["u32"]
    st = np.diff(inp["tile_first"].astype(np.int64))
    empty = st == 0
    bit_lo = c["bit_lo"]
    pad = k == np.uint32(0xFFFFFFFF)
    lonely = max_next = False
    for s in range(st.size):
        a, b = int(inp["tile_first"][s]) * T, int(inp["tile_first"][s + 1]) * T
        if b > a:
            real = int((~pad[a:b]).sum())
            lonely |= real == 1
            if real < b - a and real > 0:
                assert not pad[a:a + real].any(), "the padding is at the segment's end"
                max_next |= int((k[a + real - 1] >> np.uint32(bit_lo)) & np.uint32(0xFFFF)) == 0xFFFF
    outside = k[~pad] & ~np.uint32(0xFFFF << bit_lo)
    inner = empty[1:-1]
    return dict(nseg=int(st.size), tiles=int(st.sum()), seg_tiles=tuple(int(v) for v in st), empty_first=bool(empty[0]),
                empty_last=bool(empty[-1]), empty_middle=bool(inner.any()), empty_run=bool((empty[1:] & empty[:-1]).any()),
                lonely=bool(lonely), max_field_next_to_padding=bool(max_next), payload_varies=np.unique(outside).size > 1)
