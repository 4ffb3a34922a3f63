"""Model of one pass of the suffix sorter's finisher (k_finish of bwtc_amd/csrc/bwt_engine.hip, chars and RANK form, and
k_rank_updates), in numpy, and the named cases of tests/test_finmodel.py (no GPU) and tests/test_gpu_finisher.py.

Inputs are honest: T is built by the case, SA by suffix_array() below (prefix doubling, held to sorted() by the CPU
test), a group is a slot range [lo, hi) of SA whose members really share `depth` characters (lcp_adjacent), and C is the
predecessor byte | depth << 8.  The expectation of a pass follows from ownership and from the true order, not from the
kernel's arithmetic:

  ownership   a workgroup owns a group that starts in its first `stride` = window - group entries (of its region) and
              has at most `group` members; every other group's members are hard, each exactly once -- shallow instead
              when their depth is below `floor`.
  splitting   an owned group splits by its members' next 8 * words * rounds characters; characters past n read as zero,
              and of two members equal under that rule of which at least one reaches past n the larger suffix number
              comes first (they are never equal).  RANK: by (rank[s + at] + 1 or 0, rank[s + at2] + 1 or 0).
  finals      a member alone in its sub-group: SA[slot], out[slot] (last_char at slot out_n), pidx for suffix 0,
              lf[(n - s) / x] when x divides n - s and the quotient is in [1, lf_n).
  next list   the others: H = old head + members below, P inside [H, H + size), depth min(255, depth + chars) (RANK:
              unchanged), region (workgroup / 64) % 16.

Free on the device, so not pinned: the order of workgroups inside a region, and which member of a tied sub-group gets
which P.  canon() therefore turns a device result into sets: the hard and the shallow list as rows sorted by suffix, the
next list per region as rows (H, S, C) sorted -- the set of its groups -- after checking the invariant the next pass
relies on (equal H adjacent, P - H counting up from 0)."""
import functools

import numpy as np

NONE = 0xFFFFFFFF
POISON = 0xA5A5A5A5
REGIONS, CHUNK = 16, 64
SHAPES = [(1024, 256), (1024, 512), (2048, 256), (2048, 512), (2048, 1024)]
CONFIGS = [(2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (4, 1)]          # (words, rounds)


def suffix_array(T):
    """The suffix array of T under "proper prefix sorts first", by prefix doubling from keys of seven characters (nine bits
    each: 0 is "past the end", below every byte)."""
    T = np.asarray(T, np.uint8)
    n = T.size
    if n == 0:
        return np.zeros(0, np.uint32)
    Tp = np.zeros(n + 7, np.int64)
    Tp[:n] = T.astype(np.int64) + 1
    key = np.zeros(n, np.int64)
    for j in range(7):
        key = (key << 9) | Tp[j:j + n]
    mul = n + 2
    h = 7
    while True:
        sa = np.argsort(key, kind="stable")
        ks = key[sa]
        rank = np.empty(n, np.int64)
        rank[sa] = np.cumsum(np.concatenate(([1], (ks[1:] != ks[:-1]).astype(np.int64))))
        if int(rank.max()) == n or h >= n:
            return sa.astype(np.uint32)
        r2 = np.zeros(n, np.int64)
        r2[:n - h] = rank[h:]
        key = rank * mul + r2
        h *= 2


def padded(T, extra=640):
    return np.concatenate((np.asarray(T, np.uint8), np.zeros(extra, np.uint8)))


def lcp_adjacent(T, SA, limit):
    """lcp[k]: characters that SA[k - 1] and SA[k] share with characters past n read as zero, capped at limit; lcp[0] = 0."""
    n = len(T)
    Tp = padded(T, 8)
    a, b = SA[:-1].astype(np.int64), SA[1:].astype(np.int64)
    lcp = np.zeros(n, np.int64)
    alive = np.ones(n - 1, bool)
    for j in range(limit):
        alive &= Tp[np.minimum(a + j, n)] == Tp[np.minimum(b + j, n)]
        if not alive.any():
            break
        lcp[1:] += alive
    return lcp


def class_heads(T, SA, d):
    """head[slot]: the first slot of the suffixes that share d characters (zero padded) with SA[slot]."""
    n = len(T)
    lcp = lcp_adjacent(T, SA, d)
    starts = np.arange(n)
    starts[lcp >= d] = 0
    starts[0] = 0
    return np.maximum.accumulate(starts)


def inverse(SA):
    isa = np.empty(len(SA), np.int64)
    isa[SA] = np.arange(len(SA))
    return isa


# ---- lists ------------------------------------------------------------------------------------------------------

def build_list(T, SA, lo, hi, depth, seed=1):
    """Groups [lo[i], hi[i]) with depth[i], in that order, members shuffled inside each group -> (S, P, H, C)."""
    lo, hi, depth = (np.asarray(x, np.int64) for x in (lo, hi, depth))
    size = hi - lo
    total = int(size.sum())
    first = np.cumsum(size) - size
    gid = np.repeat(np.arange(len(lo)), size)
    j = np.arange(total) - np.repeat(first, size)
    H = np.repeat(lo, size)
    P = H + j
    rnd = np.random.RandomState(seed).randint(0, 1 << 30, total)
    order = np.lexsort((rnd, gid))                                   # a permutation inside every group
    S = np.asarray(SA, np.int64)[P[order]]
    Tn = np.asarray(T, np.uint8)
    pred = np.where(S > 0, Tn[np.maximum(S - 1, 0)], 0).astype(np.int64)
    C = pred | (np.repeat(depth, size) << 8)
    return S.astype(np.uint32), P.astype(np.uint32), H.astype(np.uint32), C.astype(np.uint16)


def place(parts, gap=37, lead=0):
    """Lists (S, P, H, C) -> arrays with one region each, `gap` unused entries between them -> (regions, S, P, H, C)."""
    regions, at = [], lead
    for p in parts:
        regions.append((at, len(p[0])))
        at += len(p[0]) + gap
    span = max([1] + [b + c for b, c in regions])
    out = [np.full(span, NONE, np.uint32), np.full(span, NONE, np.uint32), np.full(span, NONE, np.uint32), np.full(span, 0xFFFF, np.uint16)]
    for (b, c), p in zip(regions, parts):
        for k in range(4):
            out[k][b:b + c] = p[k]
    return regions, out[0], out[1], out[2], out[3]


def cut(lst, k0, k1):
    return tuple(a[k0:k1] for a in lst)


# ---- the model of one pass -----------------------------------------------------------------------------------------

def _entries(regions, S, P, H, C, stride):
    """All entries of the regions: list position q, suffix, slot, head, character field, group id, the group's start (in its
    region) and size, the workgroup (of the whole grid) whose stride range the group starts in / the entry lies in."""
    qs, wbase, w0 = [], [], 0
    for b, c in regions:
        qs.append(np.arange(b, b + c, dtype=np.int64))
        wbase.append(np.full(c, w0, np.int64))
        w0 += -(-c // stride)
    q = np.concatenate(qs) if qs else np.zeros(0, np.int64)
    wbase = np.concatenate(wbase)
    p = q - np.concatenate([np.full(c, b, np.int64) for b, c in regions])
    h = H[q].astype(np.int64)
    new = np.ones(len(q), bool)
    new[1:] = (h[1:] != h[:-1]) | (p[1:] == 0)
    gid = np.cumsum(new) - 1
    size = np.bincount(gid)
    start = p[new]
    return dict(q=q, s=S[q].astype(np.int64), slot=P[q].astype(np.int64), h=h, c=C[q].astype(np.int64), gid=gid, gsize=size[gid], gstart=start[gid],
                wg_group=wbase + start[gid] // stride, wg_entry=wbase + p // stride, grid=w0)


def expect_pass(T, regions, S, P, H, C, window=1024, group=256, words=2, rounds=1, floor=12, out_n=None, lf_n=0, rank=None, at=0, at2=0, mutant=0):
    """One pass.  mutant: the numbered mutant of DESIGN.md section 8g replayed (0: the kernel as it should be)."""
    T = np.asarray(T, np.uint8)
    n = len(T)
    out_n = n if out_n is None else out_n
    ranks = rank is not None
    stride = window - group
    chars = 8 * words * rounds
    e = _entries(regions, S, P, H, C, stride)
    depth = e["c"] >> 8
    owned = e["gsize"] <= group
    if mutant == 2:                                                # a group of group + 1 members: all but its last member pass for owned
        owned |= (e["gsize"] == group + 1) & (e["slot"] - e["h"] < group)
    res = dict(grid=e["grid"])
    # hard and shallow
    hard = ~owned & (depth >= floor)
    shal = ~owned & (depth < floor)
    for name, sel in (("hard", hard), ("shallow", shal)):
        rows = np.stack((e["s"][sel], e["h"][sel], e["slot"][sel], e["c"][sel]), 1) if sel.any() else np.zeros((0, 4), np.int64)
        rows = rows[np.argsort(rows[:, 0], kind="stable")]
        res[name] = rows if name == "hard" else rows[:, :3]
        res[name + "_count"] = (int(sel.sum()), int(depth[sel].min()) if sel.any() else NONE)
    # the owned members' keys
    o = np.flatnonzero(owned)
    s, dep = e["s"][o], depth[o]
    if ranks:
        rk = np.asarray(rank, np.int64)
        t1, t2 = s + at, s + at2
        k1 = np.where(t1 < n, rk[np.minimum(t1, n - 1)] + 1, 0)
        k2 = np.where((t2 < n) & (at2 != 0), rk[np.minimum(t2, n - 1)] + 1, 0)
        keyw = [k1, k2]
        tb = np.zeros(len(o), np.int64)
    else:
        Tp = padded(T, 8)
        pos = s + dep
        keyw = []
        for w in range(words * rounds):
            v = np.zeros(len(o), np.uint64)
            for j in range(8):
                v = (v << np.uint64(8)) | Tp[np.minimum(pos + 8 * w + j, n)].astype(np.uint64)
            keyw.append(v)
        tb = np.where(pos + chars > n, n - s, n + 1)              # reaches past n: larger suffix first, and never equal
        if mutant == 3:                                             # the smaller suffix number first
            tb = np.where(pos + chars > n, n + 2 + s, 0)
        if mutant == 4:                                             # only what the first round sees of the end of T
            tb = np.where(pos + 8 * words > n, n - s, n + 1)
    gid = e["gid"][o]
    wg_group = e["wg_group"][o]
    if mutant == 1:                                                # a group that starts on a stride is settled by the workgroup before, too
        twice = (e["gstart"][o] % stride == 0) & (e["gstart"][o] > 0)
        dup = np.flatnonzero(twice)
        o = np.concatenate((o, o[dup]))
        gid = np.concatenate((gid, gid[dup] + int(e["gid"].max()) + 1))
        wg_group = np.concatenate((wg_group, wg_group[dup] - 1))
        keyw = [np.concatenate((k, k[dup])) for k in keyw]
        tb = np.concatenate((tb, tb[dup]))
    order = np.lexsort([tb] + keyw[::-1] + [gid])
    so = o[order]
    newg = np.ones(len(so), bool)
    newg[1:] = gid[order][1:] != gid[order][:-1]
    news = newg.copy()
    for k in keyw + [tb]:
        kk = k[order]
        news[1:] |= kk[1:] != kk[:-1]
    idx = np.arange(len(so))
    gfirst = np.maximum.accumulate(np.where(newg, idx, 0))
    sfirst = np.maximum.accumulate(np.where(news, idx, 0))
    sid = np.cumsum(news) - 1
    ssize = np.bincount(sid)[sid] if len(so) else np.zeros(0, np.int64)
    below = sfirst - gfirst
    newh = e["h"][so] + below
    final = ssize == 1
    # finals
    SAx = np.full(n, POISON, np.uint32)
    outx = np.full(n, 0xA5, np.uint8)
    lf = np.full(256, POISON, np.uint32)
    fs, fslot, fc = e["s"][so][final], newh[final], e["c"][so][final] & 0xFF
    SAx[fslot] = fs
    inside = fslot < out_n
    outx[fslot[inside]] = fc[inside]
    res["last_char"] = int(fc[~inside][0]) if (~inside).any() else POISON
    res["pidx"] = int(fslot[fs == 0][0]) if (fs == 0).any() else POISON
    if lf_n > 1:
        x = n // lf_n
        t = n - fs
        hit = (t % x == 0) & (t // x >= 1) & (t // x < lf_n)
        if mutant == 7 and x > 1:                                   # the multiply-high quotient without its correction
            q = (t * ((1 << 32) // x)) >> 32
            hit &= t - q * x == 0
        lf[(t // x)[hit]] = fslot[hit]
    res.update(SA=SAx, out=outx, lf=lf)
    # the next list
    left = ~final
    newc = e["c"][so] if ranks else (e["c"][so] & 0xFF) | (np.minimum(255, (e["c"][so] >> 8) + (8 * words if mutant == 5 else chars)) << 8)
    oreg = (wg_group[order] // CHUNK) % REGIONS
    nxt, cnt = {}, np.zeros(REGIONS + 1, np.int64)
    for r in range(REGIONS):
        sel = left & (oreg == r)
        rows = np.stack((newh[sel], e["s"][so][sel], newc[sel]), 1) if sel.any() else np.zeros((0, 3), np.int64)
        nxt[r] = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
        cnt[r] = len(rows)
    cnt[REGIONS] = int((news & left).sum()) if mutant != 9 else int((~news & left).sum())
    res.update(next=nxt, next_count=cnt)
    if ranks:
        span = max(b + c for b, c in regions)
        us, ur = np.full(span, NONE, np.int64), np.full(span, POISON, np.int64)
        q = e["q"][so]
        us[q] = np.where((below > 0) | (mutant == 8), e["s"][so], NONE)
        ur[q] = newh
        rk2 = np.asarray(rank, np.int64).copy()
        upd = (below > 0) | (mutant == 8)
        rk2[e["s"][so][upd]] = newh[upd]
        res.update(us=us, ur=ur, rank=rk2)
    return res


def room_of(regions, window, group):
    stride = window - group
    grid = sum(-(-c // stride) for _, c in regions)
    return grid * stride + -(-grid // CHUNK) * group


def canon(got, n, ranks=False):
    """A device result (hip.Context.test_finish_pass) in the model's form; raises where the next list breaks the
    invariant the next pass relies on."""
    res = dict(SA=got["SA"], out=got["out"], lf=got["lf"], pidx=got["pidx"], last_char=got["last_char"])
    hS, hHP, hC = got["hard"]
    rows = np.stack((hS.astype(np.int64), (hHP >> np.uint64(32)).astype(np.int64), (hHP & np.uint64(NONE)).astype(np.int64), hC.astype(np.int64)), 1)
    res["hard"] = rows[np.argsort(rows[:, 0], kind="stable")]
    sS, sHP = got["shallow"]
    rows = np.stack((sS.astype(np.int64), (sHP >> np.uint64(32)).astype(np.int64), (sHP & np.uint64(NONE)).astype(np.int64)), 1)
    res["shallow"] = rows[np.argsort(rows[:, 0], kind="stable")]
    res["hard_count"] = (int(got["hard_count"][0]), int(got["hard_count"][1]))
    res["shallow_count"] = (int(got["shal_count"][0]), int(got["shal_count"][1]))
    nS, nP, nH, nC = got["next"]
    res["next_count"] = got["next_count"].astype(np.int64)
    nxt, regions = {}, []
    for r in range(REGIONS):
        b, c = int(got["next_base"][r]), int(got["next_count"][r])
        assert b + c <= len(nS), "region %d of the next list leaves its room" % r
        if r + 1 < REGIONS:
            assert b + c <= int(got["next_base"][r + 1]), "region %d of the next list runs into the next" % r
        regions.append((b, c))
        s, p, h, cc = (a[b:b + c].astype(np.int64) for a in (nS, nP, nH, nC))
        new = np.ones(c, bool)
        new[1:] = h[1:] != h[:-1]
        first = np.maximum.accumulate(np.where(new, np.arange(c), 0))
        assert np.array_equal(p - h, np.arange(c) - first), "next list, region %d: P - H does not count up from 0 inside a run of equal H" % r
        assert len(np.unique(h[new])) == int(new.sum()), "next list, region %d: a head in two runs" % r
        rows = np.stack((h, s, cc), 1)
        nxt[r] = rows[np.lexsort((s, h))]
    res["next"] = nxt
    res["next_regions"] = regions
    if ranks:
        res.update(us=got["us"].astype(np.int64), ur=got["ur"].astype(np.int64), rank=got["rank"].astype(np.int64))
    return res


def differences(want, have, ranks=False):
    """Names of the outputs in which two canonical results differ (exact comparison)."""
    bad = []
    for k in ("SA", "out", "lf", "hard", "shallow", "next_count") + (("us", "ur", "rank") if ranks else ()):
        a, b = np.asarray(want[k]), np.asarray(have[k])
        if a.shape != b.shape or not np.array_equal(a.astype(np.int64), b.astype(np.int64)):
            bad.append(k)
    for k in ("pidx", "last_char", "hard_count", "shallow_count"):
        if want[k] != have[k]:
            bad.append("%s: want %s, have %s" % (k, want[k], have[k]))
    for r in range(REGIONS):
        a, b = want["next"][r], have["next"][r]
        if a.shape != b.shape or not np.array_equal(a, b):
            bad.append("next[%d]" % r)
    return bad


# ---- the two properties, from the true suffix array alone ---------------------------------------------------------------

def placed_breaks(res, SA_true):
    """Finals (slot, s) with s != SA_true[slot]."""
    slots = np.flatnonzero(res["SA"] != POISON)
    return int((res["SA"][slots] != SA_true[slots]).sum())


def refined_breaks(T, SA_true, res, claim_chars=True):
    """Groups left (next list, hard, shallow) that are not a slot range holding SA_true over that range, whose members do
    not share the depth they claim, or -- next list -- that have one member only (a member whose next characters are
    unique in its old group is final)."""
    T = np.asarray(T, np.uint8)
    n = len(T)
    Tp = padded(T, 8)
    bad = 0
    lists = [res["next"][r] for r in range(REGIONS)]               # rows (H, S, C)
    lists += [res["hard"][:, [1, 0, 3]]] if len(res["hard"]) else []
    for i, rows in enumerate(lists):
        if not len(rows):
            continue
        rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
        h, s, c = rows[:, 0], rows[:, 1], rows[:, 2]
        new = np.ones(len(h), bool)
        new[1:] = h[1:] != h[:-1]
        first = np.maximum.accumulate(np.where(new, np.arange(len(h)), 0))
        slots = h + np.arange(len(h)) - first                      # the group's slots, in order
        if slots.max() >= n:
            return 1 << 30
        truth = SA_true[slots].astype(np.int64)
        tr = np.stack((h, truth), 1)
        tr = tr[np.lexsort((tr[:, 1], tr[:, 0]))]
        bad += int((tr[:, 1] != s).sum())
        size = np.bincount(np.cumsum(new) - 1)
        if i < REGIONS:
            bad += int((size < 2).sum())
        if claim_chars:
            other = np.flatnonzero(~new)                             # every member against its group's first
            d, so, lead = (c >> 8)[other], s[other], s[first][other]
            bad += int(((c >> 8) != (c >> 8)[first]).sum())
            for j in range(int(d.max()) if len(d) else 0):
                ne = (Tp[np.minimum(so + j, n)] != Tp[np.minimum(lead + j, n)]) & (j < d)
                bad += int(ne.sum())
    return bad


# ---- texts ---------------------------------------------------------------------------------------------------------------

EDGE_BYTES = np.array([0x00, 0x7F, 0x80, 0xFF], np.uint8)            # what the unsigned compare behind the byte swap must get right


@functools.lru_cache(maxsize=None)
def phrase_text(n, seed, nphr=6, plen=150, zeros_tail=0):
    """Phrases over {0x00, 0x7F, 0x80, 0xFF} in random order: repeats far longer than a pass compares, so that a pass
    leaves finals and ties; optionally ending in zero bytes."""
    r = np.random.RandomState(seed)
    phr = [EDGE_BYTES[r.randint(0, 4, plen + r.randint(0, 9))] for _ in range(nphr)]
    parts, have = [], 0
    while have < n:
        p = phr[r.randint(0, nphr)]
        parts.append(p)
        have += len(p)
    T = np.concatenate(parts)[:n].copy()
    if zeros_tail:
        T[n - zeros_tail:] = 0
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def twin_text(L, seed):
    """X + X, X random bytes: every suffix of the first half has a twin that shares all that is left of the half."""
    X = np.random.RandomState(seed).randint(0, 256, L).astype(np.uint8)
    T = np.concatenate((X, X))
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def sa_of(kind, *args):
    T = {"phrase": phrase_text, "twin": twin_text, "ab": ab_text}[kind](*args)
    return T, suffix_array(T)


@functools.lru_cache(maxsize=None)
def ab_text(n, tail):
    """abab...ab: a text that ends in its own prefix (every suffix is a prefix of the one two places before it)."""
    T = np.tile(np.array([0x61, 0x62], np.uint8), n // 2 + 1)[:n].copy()
    if tail:
        T[n - tail:] = 0
    T.setflags(write=False)
    return T


# ---- cases -----------------------------------------------------------------------------------------------------------------

def _ranges_list(T, SA, sizes, lo0, dcap, seed):
    """Consecutive slot ranges of the given sizes from slot lo0, each claiming min(what its members share, dcap)."""
    sizes = np.asarray(sizes, np.int64)
    hi = lo0 + np.cumsum(sizes)
    lo = hi - sizes
    if dcap:
        lcp = lcp_adjacent(T, SA, dcap)
        inner = lcp[:int(hi[-1])].copy()
        inner[lo] = dcap                                            # (a group's first member shares nothing with itself)
        depth = np.minimum.reduceat(inner, lo)
    else:
        depth = np.zeros(len(sizes), np.int64)
    return build_list(T, SA, lo, hi, depth, seed)


def _filler(total, seed, top=7):
    """Group sizes 1..top that sum to total."""
    r = np.random.RandomState(seed)
    out = []
    while total > 0:
        g = min(total, int(r.randint(1, top + 1)))
        out.append(g)
        total -= g
    return out


def _seam_sizes(win, G):
    """Group sizes that put each of the issue's seam situations at a chosen window position: (name, sizes)."""
    st = win - G
    f = lambda k, seed=3: _filler(k, seed)
    cs = []
    for m in (1, 2, st - 1, st, st + 1, win - 1, win, win + 1, 2 * st - 1, 2 * st + 1):
        cs.append(("list%d" % m, f(m, m)))
    cs.append(("sizes", f(5) + [1, 2, G - 1] + f(9) + [G, G + 1, 3] + [2 * G] + f(4) + [win + 1, 2, 3 * st + 5] + f(11)))
    cs.append(("sizes_rev", f(11) + [3 * st + 5, 2, win + 1] + f(4) + [2 * G, 3, G + 1, G] + f(9) + [G - 1, 2, 1] + f(5)))
    for a in (0, 1, st - 1, st, st + 1, 2 * st - 1, 2 * st, 2 * st + 1):
        for g in (2, G, G + 1):
            cs.append(("start%d_g%d" % (a, g), f(a, a + 1) + [g] + f(7)))
    cs.append(("first_last_owned", [G] + f(st + 9) + [G]))
    cs.append(("first_last_hard", [G + 1] + f(st + 9) + [G + 3]))
    cs.append(("cut_then_owned", f(st - 5) + [G, 9, 2] + f(20)))               # a group of G cut by the second window's start, an owned one behind it
    cs.append(("cut_small_then_owned", f(st - 1) + [2, G] + f(20)))
    cs.append(("cut_hard", f(st - 5) + [G + 7, 9] + f(20)))                    # a hard group cut by the window's start
    cs.append(("hard_over_strides", f(st - G) + [G + 5, 4] + f(30)))           # its first G members in one stride range, the rest in the next
    cs.append(("hard_over_three", f(st - 3) + [2 * st + 9, 4] + f(30)))
    return cs


def cases():
    """Every named case: dict(name, bucket, kind, ...) for make()."""
    cs = []
    k = 0
    for (win, G) in SHAPES:
        for name, sizes in _seam_sizes(win, G):
            words, rounds = CONFIGS[k % len(CONFIGS)]
            cs.append(dict(bucket="seams-%d-%d" % (win, G), name="seam-%d-%d-%s" % (win, G, name), kind="ranges", sizes=sizes, win=win, G=G, words=words,
                           rounds=rounds, floor=(0, 12, 48)[k % 3], dcap=(0, 40, 60)[(k // 3) % 3], seed=k, nreg=1))
            k += 1
    # regions: the same lists cut into 2 and 16 regions with empty ones among them, a region of one group, one that ends on a stride
    for (win, G) in SHAPES:
        st = win - G
        sizes = _filler(3 * st + 11, 5, top=9) + [G + 2] + _filler(st, 6)
        for nreg, cuts in ((2, "mid"), (16, "spread"), (16, "one_group"), (3, "on_stride")):
            words, rounds = CONFIGS[k % len(CONFIGS)]
            cs.append(dict(bucket="regions", name="regions-%d-%d-%d-%s" % (win, G, nreg, cuts), kind="ranges", sizes=sizes, win=win, G=G, words=words,
                           rounds=rounds, floor=12, dcap=40, seed=k, nreg=nreg, cuts=cuts))
            k += 1
    # the dealing of the output: every group left tied, grids of 64, 65, 1024 and 1025 workgroups
    for (win, G), grids in (((1024, 256), (64, 65, 1024, 1025)), ((2048, 1024), (64, 65, 1024, 1025))):
        for grid in grids:
            cs.append(dict(bucket="dealing-%d" % win, name="dealing-%d-%d-grid%d" % (win, G, grid), kind="twins", win=win, G=G, grid=grid, words=2, rounds=1,
                           floor=12, seed=grid))
    cs += _char_cases() + _end_cases() + _depth_cases() + _emit_cases() + _rank_cases()
    return cs


def buckets(prefix=""):
    seen = []
    for c in cases():
        if c["bucket"].startswith(prefix) and c["bucket"] not in seen:
            seen.append(c["bucket"])
    return seen


_PREFIX = np.array([0xF1, 0xE2, 0xD3, 0xC4, 0xB5, 0xA6, 0x97, 0x88, 0x79, 0x6A], np.uint8)


def _sep(i, k):
    """A separator of 3 + k bytes that no other record has (bytes 0x01 .. 0x3F only)."""
    return np.array([1 + (i % 60), 1 + (i // 60) % 60, 0x3F] + [0x20] * k, np.uint8)


def _char_cases():
    """Members that differ in one chosen byte of what a pass compares, or in none: see make()."""
    cs = []
    for ci, (words, rounds) in enumerate(CONFIGS):
        win, G = SHAPES[ci % len(SHAPES)]
        cs.append(dict(bucket="chars", name="chars-w%d-r%d" % (words, rounds), kind="chars", win=win, G=G, words=words, rounds=rounds, floor=12, end=False))
        cs.append(dict(bucket="chars", name="chars-w%d-r%d-end" % (words, rounds), kind="chars", win=win, G=G, words=words, rounds=rounds, floor=12, end=True))
    return cs


def _end_cases():
    cs = []
    for ci, (words, rounds) in enumerate(CONFIGS):
        win, G = SHAPES[(ci + 2) % len(SHAPES)]
        chars = 8 * words * rounds
        for left in range(0, chars + 2):
            cs.append(dict(bucket="end-w%d-r%d" % (words, rounds), name="end-w%d-r%d-left%d" % (words, rounds, left), kind="end", win=win, G=G, words=words,
                           rounds=rounds, floor=12, left=left))
        for past in (1, 5):
            cs.append(dict(bucket="end-w%d-r%d" % (words, rounds), name="end-w%d-r%d-past%d" % (words, rounds, past), kind="end", win=win, G=G, words=words,
                           rounds=rounds, floor=12, left=-past))
    for n, tail in ((501, 0), (500, 0), (777, 40), (2300, 0)):
        for ci, (words, rounds) in enumerate(CONFIGS[1::2]):
            win, G = SHAPES[(ci + n) % len(SHAPES)]
            cs.append(dict(bucket="end-texts", name="end-ab-%d-%d-w%d-r%d" % (n, tail, words, rounds), kind="ab", n=n, tail=tail, win=win, G=G, words=words,
                           rounds=rounds, floor=0))
    for ci, (words, rounds) in enumerate(CONFIGS):
        win, G = SHAPES[ci % len(SHAPES)]
        cs.append(dict(bucket="end-texts", name="end-zeros-w%d-r%d" % (words, rounds), kind="ranges", sizes=_filler(1500, ci), win=win, G=G, words=words,
                       rounds=rounds, floor=0, dcap=0, seed=ci, nreg=1, zeros_tail=300, lo0=0))
    return cs


def _depth_cases():
    cs = []
    for ci, (words, rounds) in enumerate(CONFIGS):
        chars = 8 * words * rounds
        for floor in (0, 12, 48):
            win, G = ((1024, 256), (2048, 256))[(ci + floor // 12) % 2]   # (a hard group is G + 1 records of text: the narrow bound)
            cs.append(dict(bucket="depths", name="depths-w%d-r%d-floor%d" % (words, rounds, floor), kind="depths", win=win, G=G, words=words, rounds=rounds,
                           floor=floor, depths=sorted(set([0, 1, max(floor - 1, 0), floor, 48, 254 - chars, 255 - chars, 256 - chars, 255]))))
    return cs


def _emit_cases():
    cs = []
    k = 0
    for lf_n, n in ((0, 3001), (1, 3001), (2, 3001), (8, 3000), (8, 3001), (8, 16), (8, 24), (256, 256), (256, 512), (256, 768), (256, 256 * 16), (256, 256 * 13 + 57),
                    (5, 4099), (2, 2), (3, 10)):
        for out_n_less in (0, 1):
            words, rounds = CONFIGS[k % len(CONFIGS)]
            win, G = SHAPES[k % len(SHAPES)]
            cs.append(dict(bucket="emit", name="emit-lf%d-n%d-%d" % (lf_n, n, out_n_less), kind="emit", n=n, lf_n=lf_n, out_n_less=out_n_less, win=win, G=G,
                           words=words, rounds=rounds, floor=0, seed=k))
            k += 1
    return cs


def _rank_cases():
    cs = []
    k = 0
    for (win, G) in SHAPES:
        for at2_on in (0, 1):
            for h in (1, 4, 16):
                cs.append(dict(bucket="rank", name="rank-%d-%d-at%d-two%d" % (win, G, h, at2_on), kind="rank", win=win, G=G, at=h, at2_on=at2_on, n=1500 + 77 * k,
                               seed=k, nreg=(1, 2, 16)[k % 3], text="phrase"))
                k += 1
    for at2_on in (0, 1):                                               # rank[] as deep as it gets (the inverse suffix array): a look-up meets rank n - 1
        cs.append(dict(bucket="rank", name="rank-top-two%d" % at2_on, kind="rank", win=1024, G=256, at=4, at2_on=at2_on, n=2600, seed=k, nreg=2, text="phrase",
                       deep=True))
        k += 1
    for n in (300, 301):
        for at2_on in (0, 1):
            cs.append(dict(bucket="rank", name="rank-ab-%d-two%d" % (n, at2_on), kind="rank", win=1024, G=256, at=2, at2_on=at2_on, n=n, seed=k, nreg=1, text="ab"))
            k += 1
    for entries in (2, 1023, 1024, 1025):
        for nreg in (2, 16):
            cs.append(dict(bucket="rank-updates", name="rank-updates-%d-regions%d" % (entries, nreg), kind="rank", win=1024, G=256, at=3, at2_on=1, n=40000,
                           seed=k, nreg=nreg, text="phrase", per_region=entries))
            k += 1
    return cs


def _split_regions(lst, sizes, nreg, cuts, stride):
    """The list cut at group boundaries into nreg regions (some empty) -> parts for place()."""
    ends = np.cumsum(sizes)
    total = int(ends[-1])
    if nreg == 1:
        return [lst]
    if cuts == "mid":
        at = [int(ends[len(ends) // 2])]
    elif cuts == "one_group":
        at = [int(ends[3]), int(ends[4])]                               # the fifth group alone
    elif cuts == "on_stride":
        k = int(np.searchsorted(ends, 2 * stride))
        at = [int(ends[k])] if ends[k] % stride == 0 else None
    else:
        at = [int(ends[i]) for i in np.linspace(2, len(ends) - 3, 7).astype(int)]
    if at is None:
        raise AssertionError("no group ends on a stride")
    bounds = [0] + at + [total]
    parts = [cut(lst, bounds[i], bounds[i + 1]) for i in range(len(bounds) - 1)]
    empty = cut(lst, 0, 0)
    out = []
    for i, p in enumerate(parts):                                       # empty regions first, between and last
        if len(out) + (len(parts) - i) < nreg:
            out.append(empty)
        out.append(p)
    while len(out) < nreg:
        out.append(empty)
    return out[:nreg] if len(out) > nreg else out


def make(c):
    """-> dict(T, SA, regions, S, P, H, C, and the keyword arguments of a pass in `args`; rank / at / at2 for RANK)."""
    kind = c["kind"]
    args = dict(window=c["win"], group=c["G"], words=c.get("words", 2), rounds=c.get("rounds", 1), floor=c.get("floor", 12))
    stride = c["win"] - c["G"]
    extra = {}
    if kind == "ranges":
        sizes = list(c["sizes"])
        if c.get("cuts") == "on_stride":                                # make the group that crosses 2 * stride end there
            ends = np.cumsum(sizes)
            k = int(np.searchsorted(ends, 2 * stride))
            over = int(ends[k]) - 2 * stride
            if over:
                sizes[k] -= over
                sizes.insert(k + 1, over)
        total = sum(sizes)
        n = total + 300 + c["seed"] % 7
        T, SA = sa_of("phrase", n, 11 + c["seed"] % 3, 6, 150, c.get("zeros_tail", 0))
        lo0 = c.get("lo0", (n - total) // 2)
        lst = _ranges_list(T, SA, sizes, lo0, c["dcap"], c["seed"])
        parts = _split_regions(lst, sizes, c["nreg"], c.get("cuts"), stride)
        regions, S, P, H, C = place(parts, lead=c["seed"] % 5)
    elif kind == "twins":
        want = c["grid"] * stride - (stride // 2)                       # entries: the last workgroup half full
        lst, T, SA = twin_list(want // 2, (65 if c["grid"] <= 65 else 1025) * stride // 2, c["seed"])
        regions, S, P, H, C = place([lst])
    elif kind in ("chars", "end", "depths"):
        T, SA, groups = _designed(c)
        lo, hi, dep = zip(*groups)
        lst = build_list(T, SA, lo, hi, dep, 5)
        regions, S, P, H, C = place([lst], lead=3)
    elif kind == "ab":
        T, SA = sa_of("ab", c["n"], c["tail"])
        n = len(T)
        sizes = _filler(n, c["n"], top=40)
        lst = _ranges_list(T, SA, sizes, 0, 200, 3)
        regions, S, P, H, C = place([lst])
    elif kind == "emit":
        n = c["n"]
        T, SA = sa_of("phrase", n, 21 + c["seed"], 6, 40, 0)
        sizes = _filler(n, c["seed"], top=5)                            # every suffix is on the list: suffix 0, slot n - 1, every n - k x
        lst = _ranges_list(T, SA, sizes, 0, 30, c["seed"])
        regions, S, P, H, C = place([lst])
        args.update(lf_n=c["lf_n"], out_n=n - c["out_n_less"])
    elif kind == "rank":
        T, SA, regions, S, P, H, C, extra = _rank_inputs(c)
        args = dict(window=c["win"], group=c["G"], floor=0)
    else:
        raise KeyError(kind)
    return dict(T=T, SA=SA, regions=regions, S=S, P=P, H=H, C=C, args=args, **extra)


def _assemble(fams, tail=None):
    """fams: [(bodies, claimed depth)] -> record text (a family's records start with a tag of 12 bytes nothing else
    starts with), its suffix array and the families as groups [(lo, hi, depth)], each checked to be one slot range."""
    parts, fam_starts, at, ri = [], [], 0, 0
    for fi, (bodies, _) in enumerate(fams):
        tag = np.concatenate((_PREFIX, np.array([0x41 + fi // 50, 0x41 + fi % 50], np.uint8)))
        st = []
        for b in bodies:
            st.append(at)
            rec = np.concatenate((tag, np.asarray(b, np.uint8), _sep(ri, ri % 8)))
            parts.append(rec)
            at += len(rec)
            ri += 1
        fam_starts.append(st)
    if tail is not None:                                                 # a last record without a separator: the text ends in it
        fam, rec = tail
        fam_starts[fam].append(at)
        parts.append(np.asarray(rec, np.uint8))
    T = np.concatenate(parts)
    T.setflags(write=False)
    SA = suffix_array(T)
    isa = inverse(SA)
    groups = []
    for (bodies, d), st in zip(fams, fam_starts):
        slots = np.sort(isa[np.array(st, np.int64)])
        assert slots[-1] - slots[0] + 1 == len(slots), "a family is not one slot range"
        groups.append((int(slots[0]), int(slots[-1]) + 1, int(d)))
    return T, SA, groups


def _tag(fi):
    return np.concatenate((_PREFIX, np.array([0x41 + fi // 50, 0x41 + fi % 50], np.uint8)))


def _designed(c):
    words, rounds, kind = c["words"], c["rounds"], c["kind"]
    chars, kr = 8 * words * rounds, 8 * words
    base = EDGE_BYTES[np.random.RandomState(chars).randint(0, 4, 900)]
    fams, tail = [], None
    if kind == "chars":
        spots = sorted(set([r * kr for r in range(rounds)] + [(r + 1) * kr - 1 for r in range(rounds)] + [7, 8]))
        for sp in spots:                                                # apart in one byte only: 0x00 < 0x7F < 0x80 < 0xFF, some of them twice
            bodies = []
            for v in (0x80, 0x00, 0xFF, 0x7F, 0x80, 0xFF, 0xFF):
                b = base[:chars + 40].copy()
                b[sp] = v
                bodies.append(b)
            fams.append((bodies, 12))
        fams.append(([base[:chars + 40]] * 9, 12))                      # the whole group equal
        fams.append(([np.roll(base[:chars + 40], i) for i in range(1, 12)], 12))   # (nearly) all distinct
        again = []                                                      # sub-groups that split again in every later round
        for i in range(2 ** rounds):
            b = base[:chars + 40].copy()
            for r in range(rounds):
                b[r * kr + 3] = 0x10 + ((i >> r) & 1)
            again += [b, b, b] if i % 3 == 0 else [b, b] if i % 3 == 1 else [b]
        fams.append((again, 12))
        if c.get("end"):                                                # one member of the window reaches past the end: the other loop
            fams.append(([base[:5], base[:5]], 12))
            tail = (len(fams) - 1, np.concatenate((_tag(len(fams) - 1), base[:5])))
    elif kind == "end":
        left = c["left"]
        r = np.random.RandomState(7)
        fams.append(([base[100 + 9 * i:160 + 9 * i + i] for i in range(5)], 12))     # other groups of the window
        fi = len(fams)
        zeros = np.zeros(chars + 8, np.uint8)
        if left >= 0:
            body = base[:left]
            fams.append(([np.concatenate((body, zeros)), np.concatenate((body, zeros)), np.concatenate((body, [1, 2, 3]))], 12))
            tail = (fi, np.concatenate((_tag(fi), body)))
        else:
            zp = np.zeros(-left, np.uint8)                              # the members' tags end where the text does: zero bytes where the last one ran out
            fams.append(([], 12))
            T0, SA0, groups = _assemble(fams[:1])
            recs = [np.concatenate((_tag(fi)[:12 + left], zp, zeros, _sep(90 + i, i))) for i in range(2)] + [np.concatenate((_tag(fi)[:12 + left], zp, [5], _sep(93, 1)))]
            T = np.concatenate([T0] + recs + [_tag(fi)[:12 + left]])
            T.setflags(write=False)
            SA = suffix_array(T)
            isa = inverse(SA)
            at, st = len(T0), []
            for rec in recs:
                st.append(at)
                at += len(rec)
            st.append(at)
            slots = np.sort(isa[np.array(st)])
            assert slots[-1] - slots[0] + 1 == len(slots)
            first = np.sort(isa[np.array([int(SA0[k]) for k in range(groups[0][0], groups[0][1])])])
            assert first[-1] - first[0] + 1 == len(first)
            return T, SA, [(int(first[0]), int(first[-1]) + 1, 12), (int(slots[0]), int(slots[-1]) + 1, 12)]
    elif kind == "depths":
        A, B = base[300:330 + chars], base[400:430 + chars]
        Cc = A.copy()
        Cc[chars - 1] ^= 0x80
        for d in c["depths"]:
            common = base[:max(d - 12, 0)]
            fams.append(([np.concatenate((common, t)) for t in (A, A, B, Cc)], d))
        floor = c["floor"]
        hard = ([floor - 1] if floor else []) + [floor + 1, max(48, floor + 2), floor]     # the smallest depth of the hard list: its last entries
        for k, d in enumerate(hard):
            common = base[:max(d - 12, 0)]
            fams.append(([np.concatenate((common, [0x30 + i % 3])) for i in range(c["G"] + 1 + k)], d))
    T, SA, groups = _assemble(fams, tail)
    return T, SA, groups


def _rank_inputs(c):
    """A RANK pass: the groups are pieces (2 .. G members) of the classes that share `at` characters, rank[] the head
    slot of every suffix's class at depth `at` (what the engine's rank[] is at least), at2 = 2 at or 0."""
    n, at, G = c["n"], c["at"], c["G"]
    if c["text"] == "ab":
        T, SA = sa_of("ab", n, 0)
    else:
        T, SA = sa_of("phrase", n, 31 + c["seed"] % 4, 6, 150, 0)
    heads = class_heads(T, SA, at)
    isa = inverse(SA)
    rank = isa if c.get("deep") else heads[isa]
    starts = np.flatnonzero(heads == np.arange(n))
    ends = np.concatenate((starts[1:], [n]))
    r = np.random.RandomState(c["seed"])
    per = c.get("per_region")
    pieces = []
    for lo, hi in zip(starts, ends):
        while hi - lo >= 2:
            if per:
                g = 3 if hi - lo == 3 else 2
            else:
                g = int(min(hi - lo, [2, 3, 5, G - 1, G, int(r.randint(2, 40))][r.randint(0, 6)]))
                if hi - lo - g == 1:
                    g += 1 if g < G else -1
            pieces.append((lo, lo + g))
            lo += g
    if per:
        pairs = [p for p in pieces if p[1] - p[0] == 2]
        triples = [p for p in pieces if p[1] - p[0] == 3]
        parts = []
        for _ in range(c["nreg"]):
            take = [triples.pop()] if per % 2 else []
            take += [pairs.pop() for _ in range((per - (3 if per % 2 else 0)) // 2)]
            parts.append(take)
    else:
        r.shuffle(pieces)
        nparts = {1: 1, 2: 2, 16: 9}[c["nreg"]]
        k = -(-len(pieces) // nparts)
        parts = [pieces[i * k:(i + 1) * k] for i in range(nparts)]
        while len(parts) < c["nreg"]:                                   # empty regions among them
            parts.insert(int(r.randint(0, len(parts) + 1)), [])
    lists = []
    for i, ps in enumerate(parts):
        lo = np.array([p[0] for p in ps], np.int64)
        hi = np.array([p[1] for p in ps], np.int64)
        lists.append(build_list(T, SA, lo, hi, np.full(len(ps), min(at, 255), np.int64), c["seed"] + i))
    regions, S, P, H, C = place(lists, lead=c["seed"] % 4)
    return T, SA, regions, S, P, H, C, dict(rank=rank.astype(np.uint32), at=at, at2=2 * at if c["at2_on"] else 0)


def run_model(c, inp, mutant=0):
    extra = {k: inp[k] for k in ("rank", "at", "at2") if k in inp}
    return expect_pass(inp["T"], inp["regions"], inp["S"], inp["P"], inp["H"], inp["C"], **inp["args"], **extra, mutant=mutant)


def list_breaks(T, SA_true, regions, S, P, H, C):
    """An input list held to the true suffix array: groups that are not slot ranges holding SA_true over the range or whose
    members do not share the depth they carry, plus entries whose character is not their predecessor's."""
    T = np.asarray(T, np.uint8)
    rows = [np.stack((H[b:b + c].astype(np.int64), S[b:b + c].astype(np.int64), C[b:b + c].astype(np.int64)), 1) for b, c in regions if c]
    rows = np.concatenate(rows)
    fake = dict(next={r: (rows if r == 0 else np.zeros((0, 3), np.int64)) for r in range(REGIONS)}, hard=np.zeros((0, 4), np.int64))
    bad = refined_breaks(T, SA_true, fake) - int((np.bincount(np.unique(rows[:, 0], return_inverse=True)[1]) < 2).sum())
    s = rows[:, 1]
    bad += int(((rows[:, 2] & 0xFF) != np.where(s > 0, T[np.maximum(s - 1, 0)], 0)).sum())
    return bad


def slow_pass(T, regions, S, P, H, C, window, group, words, rounds, floor, **_):
    """One chars pass by sorted() over Python byte strings, group by group -> (finals {slot: s}, per region the set of groups
    (H, C, frozenset(S)), hard set, shallow set)."""
    Tb = bytes(np.asarray(T, np.uint8))
    n = len(Tb)
    stride, chars = window - group, 8 * words * rounds
    finals, nxt, hard, shal = {}, [set() for _ in range(REGIONS)], set(), set()
    w0 = 0
    for b, c in regions:
        i = 0
        while i < c:
            j = i
            while j + 1 < c and H[b + j + 1] == H[b + i]:
                j += 1
            members = [(int(S[b + k]), int(P[b + k]), int(C[b + k])) for k in range(i, j + 1)]
            head, depth = int(H[b + i]), members[0][2] >> 8
            if len(members) > group:
                for s, p, cc in members:
                    (shal if depth < floor else hard).add((s, head, p) if depth < floor else (s, head, p, cc))
            else:
                def key(m):
                    pos = m[0] + depth
                    k = Tb[pos:pos + chars].ljust(chars, b"\0") if pos < n else bytes(chars)
                    return (k, 0, -m[0]) if pos + chars > n else (k, 1, 0)
                ms = sorted(members, key=key)
                a = 0
                while a < len(ms):
                    z = a
                    while z + 1 < len(ms) and key(ms[z + 1]) == key(ms[a]):
                        z += 1
                    if z == a:
                        finals[head + a] = ms[a][0]
                    else:
                        cc = (ms[a][2] & 0xFF) | (min(255, depth + chars) << 8)
                        assert all((m[2] & 0xFF00) == (ms[a][2] & 0xFF00) for m in ms[a:z + 1])
                        nxt[((w0 + i // stride) // CHUNK) % REGIONS].add((head + a, frozenset((m[0], (m[2] & 0xFF) | (cc & 0xFF00)) for m in ms[a:z + 1])))
                    a = z + 1
            i = j + 1
        w0 += -(-c // stride)
    return finals, nxt, hard, shal


def as_sets(res):
    """A canonical result in slow_pass's form."""
    slots = np.flatnonzero(res["SA"] != POISON)
    finals = {int(k): int(res["SA"][k]) for k in slots}
    nxt = []
    for r in range(REGIONS):
        groups = {}
        for h, s, c in res["next"][r].tolist():
            groups.setdefault(h, set()).add((s, c))
        nxt.append(set((h, frozenset(v)) for h, v in groups.items()))
    return finals, nxt, set(map(tuple, res["hard"].tolist())), set(map(tuple, res["shallow"].tolist()))


# ---- the driver, finisher_passes ------------------------------------------------------------------------------------------

def _relist(res):
    """The list a pass leaves, as one region (the order of its groups is free): rows (H, S, C) -> (S, P, H, C)."""
    rows = np.concatenate([res["next"][r] for r in range(REGIONS)])
    rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
    h = rows[:, 0]
    new = np.ones(len(h), bool)
    new[1:] = h[1:] != h[:-1]
    first = np.maximum.accumulate(np.where(new, np.arange(len(h)), 0))
    return rows[:, 1].astype(np.uint32), (h + np.arange(len(h)) - first).astype(np.uint32), h.astype(np.uint32), rows[:, 2].astype(np.uint16)


def expect_driver(T, S, P, H, C, window=1024, group=256, words=2, rounds=3, floor=12, keep_local=True, max_passes=8, out_n=None, lf_n=0, fin_max_passes=8):
    """finisher_passes restated: the model's own pass iterated under the driver's stop rules (fewer than 4096 entries left;
    more than 3/5 of the list kept, and more than n / 64 entries, from the second pass on; more than 3/4 kept from the third;
    (255 - 48) / chars passes at most; max_passes), then the want_local rule or k_fin_to_hard (whose shallow entries leave
    holes in a list no pass has looked at).  Ownership in a later pass depends on where the device put the groups, the
    outcome does not: a group of at most `group` members is somebody's wherever it lies."""
    n = len(T)
    pass_chars = 8 * words * (rounds if words == 2 else 1)
    limit = min(fin_max_passes, max(1, (255 - 48) // pass_chars), max_passes)
    lst = (np.asarray(S), np.asarray(P), np.asarray(H), np.asarray(C))
    m = len(lst[0])
    SAx, outx, lf = np.full(n, POISON, np.uint32), np.full(n, 0xA5, np.uint8), np.full(256, POISON, np.uint32)
    pidx = last_char = POISON
    hard, shallow, hard_depth = [], [], NONE
    passes, route, groups_left, stop, it = 0, 0, 0, "limit", 0
    while it < limit and m > 0:
        res = expect_pass(T, [(0, m)], *lst, window=window, group=group, words=words, rounds=rounds if words == 2 else 1, floor=floor, out_n=out_n, lf_n=lf_n)
        route |= 2
        fin = res["SA"] != POISON
        SAx[fin], outx[fin] = res["SA"][fin], res["out"][fin]
        lf[res["lf"] != POISON] = res["lf"][res["lf"] != POISON]
        pidx = res["pidx"] if res["pidx"] != POISON else pidx
        last_char = res["last_char"] if res["last_char"] != POISON else last_char
        hard.append(res["hard"][:, :3])
        hard_depth = min(hard_depth, res["hard_count"][1])
        shallow.append(res["shallow"])
        m_was, groups_left = m, int(res["next_count"][REGIONS])
        lst = _relist(res)
        m = len(lst[0])
        passes = it + 1
        if m < 4096:
            stop = "few"
            break
        if it >= 1 and m * 5 > m_was * 3 and m * 64 > n:
            stop = "three fifths"
            break
        if it >= 2 and m * 4 > m_was * 3:
            stop = "three quarters"
            break
        it += 1
    hard = np.concatenate(hard) if hard else np.zeros((0, 3), np.int64)
    shallow = np.concatenate(shallow) if shallow else np.zeros((0, 3), np.int64)
    out = dict(passes_done=passes, route=route, stop=stop, hard_depth=hard_depth, SA=SAx, out=outx, lf=lf, pidx=pidx, last_char=last_char)
    s_l, p_l, h_l, c_l = (a.astype(np.int64) for a in lst)
    left_rows = np.stack((s_l, h_l, p_l), 1) if m else np.zeros((0, 3), np.int64)
    d_l = c_l >> 8
    want_local = bool(m and keep_local and passes >= 1 and m * 64 >= n and groups_left * 24 >= m)
    holes, wait_depth = 0, NONE
    if want_local:
        rows = np.stack((h_l, s_l, c_l), 1)
        out.update(left=0, local=m, local_depth=int(d_l.min()), local_rows=rows[np.lexsort((s_l, h_l))], park=hard)
    else:
        keep = np.ones(m, bool)
        if m and passes == 0:
            keep = d_l >= floor
            shallow = np.concatenate((shallow, left_rows[~keep]))
            holes = int((~keep).sum())
        if keep.any():
            wait_depth = int(d_l[keep].min())
        out.update(left=m, local=0, local_depth=0, local_rows=np.zeros((0, 3), np.int64), park=np.concatenate((hard, left_rows[keep])))
    out.update(hard=len(hard), parked=len(hard) + (0 if want_local else m), park_holes=holes, shallow=len(shallow), wait_depth=wait_depth)
    out["park"] = out["park"][np.argsort(out["park"][:, 0], kind="stable")]
    out["shal"] = shallow[np.argsort(shallow[:, 0], kind="stable")]
    return out


def canon_driver(got):
    """A device result of hip.Context.test_finisher in expect_driver's form."""
    out = {k: got[k] for k in ("passes_done", "route", "SA", "out", "lf", "pidx", "last_char", "left", "local", "local_depth", "hard", "hard_depth", "parked", "park_holes",
                               "shallow", "wait_depth")}
    for name in ("park", "shal"):
        s, hp = got[name]
        rows = np.stack((s.astype(np.int64), (hp >> np.uint64(32)).astype(np.int64), (hp & np.uint64(NONE)).astype(np.int64)), 1)
        hole = (rows[:, 0] == NONE) & (rows[:, 1] == NONE) & (rows[:, 2] == NONE)
        if name == "park":
            out["holes_seen"] = int(hole.sum())
        rows = rows[~hole]
        out[name] = rows[np.argsort(rows[:, 0], kind="stable")]
    s, p, h, c = (a.astype(np.int64) for a in got["local_list"])
    new = np.ones(len(h), bool)
    new[1:] = h[1:] != h[:-1]
    first = np.maximum.accumulate(np.where(new, np.arange(len(h)), 0)) if len(h) else np.zeros(0, np.int64)
    assert np.array_equal(p - h, np.arange(len(h)) - first), "local list: P - H does not count up from 0 inside a run of equal H"
    rows = np.stack((h, s, c), 1)
    out["local_rows"] = rows[np.lexsort((s, h))]
    return out


def driver_refined_breaks(T, SA_true, res):
    """refined_breaks for a driver's result: the local list with the depths it claims, the parked and the shallow raw
    lists (S, H, P; no depth) as slot ranges that hold SA_true."""
    none = np.zeros((0, 3), np.int64)
    bad = refined_breaks(T, SA_true, dict(next={r: (res["local_rows"] if r == 0 else none) for r in range(REGIONS)}, hard=np.zeros((0, 4), np.int64)))
    for rows in (res["park"], res["shal"]):
        if len(rows):
            hard = np.stack((rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 0] * 0), 1)
            bad += refined_breaks(T, SA_true, dict(next={r: none for r in range(REGIONS)}, hard=hard), claim_chars=False)
    return bad


def driver_differences(want, have):
    bad = []
    for k in ("passes_done", "route", "pidx", "last_char", "left", "local", "local_depth", "hard", "hard_depth", "parked", "park_holes", "shallow", "wait_depth"):
        if int(want[k]) != int(have[k]):
            bad.append("%s: want %s, have %s" % (k, want[k], have[k]))
    if have.get("holes_seen", want["park_holes"]) != want["park_holes"]:
        bad.append("holes in the parked list: want %d, have %d" % (want["park_holes"], have["holes_seen"]))
    for k in ("SA", "out", "lf", "local_rows"):
        a, b = np.asarray(want[k]).astype(np.int64), np.asarray(have[k]).astype(np.int64)
        if a.shape != b.shape or not np.array_equal(a, b):
            bad.append(k)
    for k in ("park", "shal"):                                      # raw lists (S, H, P): which tied member holds which slot of its group is free
        a, b = np.asarray(want[k]).astype(np.int64), np.asarray(have[k]).astype(np.int64)
        if a.shape != b.shape or not np.array_equal(a[:, :2], b[:, :2]):
            bad.append(k + ": suffixes and heads")
        elif not np.array_equal(a[np.lexsort((a[:, 2], a[:, 1]))][:, 1:], b[np.lexsort((b[:, 2], b[:, 1]))][:, 1:]):
            bad.append(k + ": slots")
    return bad


@functools.lru_cache(maxsize=None)
def block_text(nblocks, blen, seed):
    """X + X with its blocks in reverse order, X random bytes: the suffixes at offset o of a block and of its copy share
    blen - o characters, no more (their followers differ)."""
    X = np.random.RandomState(seed).randint(0, 256, nblocks * blen).astype(np.uint8)
    T = np.concatenate((X, X.reshape(nblocks, blen)[::-1].ravel()))
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def _block_sa(nblocks, blen, seed):
    T = block_text(nblocks, blen, seed)
    return T, suffix_array(T)


TWIN_BLOCK, TWIN_OFFSETS = 128, 76


def twin_list(pairs, pairs_room, seed):
    """`pairs` groups of two suffixes that share 52 to 128 characters and no more (offsets 0 .. 75 of a block of
    block_text and of its copy), claimed depth 13: tied through two passes of 16 characters.  The text has room for
    pairs_room pairs (one text, and one suffix array, for the lists of a kind).  -> ((S, P, H, C), T, SA)"""
    nb = -(-pairs_room // TWIN_OFFSETS) + 8
    T, SA = _block_sa(nb, TWIN_BLOCK, 7)
    isa = inverse(SA)
    offs = np.arange(TWIN_OFFSETS, dtype=np.int64)
    s1 = (np.arange(nb)[:, None] * TWIN_BLOCK + offs[None, :]).ravel()
    s2 = (nb * TWIN_BLOCK + (nb - 1 - np.arange(nb))[:, None] * TWIN_BLOCK + offs[None, :]).ravel()
    ok = np.abs(isa[s1] - isa[s2]) == 1                                 # (nothing sorts between the two)
    lo = np.sort(np.minimum(isa[s1], isa[s2])[ok])[:pairs]
    assert len(lo) == pairs
    return build_list(T, SA, lo, lo + 2, np.full(pairs, 13, np.int64), seed), T, SA


def driver_cases():
    cs = []
    for i, (win, G) in enumerate(SHAPES):
        for keep_local in (0, 1):
            cs.append(dict(name="driver-few-%d-%d-local%d" % (win, G, keep_local), src="seam-%d-%d-sizes" % (win, G), drv=dict(keep_local=keep_local, max_passes=8),
                           stop="few", passes=1))
    cs.append(dict(name="driver-no-pass-holes", src="depths-w2-r1-floor12", drv=dict(keep_local=1, max_passes=0), stop="limit", passes=0))
    cs.append(dict(name="driver-no-pass-floor0", src="depths-w2-r1-floor0", drv=dict(keep_local=1, max_passes=0), stop="limit", passes=0))
    for keep_local in (0, 1):
        cs.append(dict(name="driver-three-fifths-local%d" % keep_local, twin=(5000, 4300), shape=(1024, 256), cfg=(2, 1), drv=dict(keep_local=keep_local, max_passes=8),
                       stop="three fifths", passes=2))
    cs.append(dict(name="driver-three-quarters", twin=(170000, 2500), shape=(2048, 512), cfg=(2, 1), drv=dict(keep_local=1, max_passes=8), stop="three quarters", passes=3))
    cs.append(dict(name="driver-max-passes", twin=(5000, 4300), shape=(1024, 512), cfg=(3, 1), drv=dict(keep_local=0, max_passes=1), stop="limit", passes=1))
    cs.append(dict(name="driver-wide", twin=(5000, 4300), shape=(2048, 1024), cfg=(2, 3), drv=dict(keep_local=1, max_passes=1), stop="limit", passes=1))
    cs.append(dict(name="driver-depth-passes", blocks=(256, 400), shape=(1024, 256), cfg=(2, 4), drv=dict(keep_local=1, max_passes=8), stop="limit", passes=3))
    cs.append(dict(name="driver-sixteen-regions", blocktwins=393408, shape=(1024, 256), cfg=(2, 1), drv=dict(keep_local=1, max_passes=8),
                   stop="three fifths", passes=2))
    return cs


def make_driver(c):
    if "src" in c:
        src = [x for x in cases() if x["name"] == c["src"]][0]
        inp = make(src)
        b, cnt = inp["regions"][0]
        a = inp["args"]
        lst = tuple(inp[k][b:b + cnt] for k in "SPHC")
        args = dict(window=a["window"], group=a["group"], words=a["words"], rounds=a["rounds"] if a["words"] == 2 else 1, floor=a["floor"])
        T, SA = inp["T"], inp["SA"]
    elif "twin" in c:
        L, pairs = c["twin"]
        T, SA = sa_of("twin", L, 7)
        sa = SA.astype(np.int64)
        pair = (np.abs(sa[1:] - sa[:-1]) == L) & (np.minimum(sa[1:], sa[:-1]) < L - 300)      # tied through every pass the driver makes
        pair[1:] &= ~pair[:-1]
        lo = np.flatnonzero(pair)[:pairs]
        assert len(lo) == pairs
        lst = build_list(T, SA, lo, lo + 2, np.full(pairs, 13, np.int64), 3)
        args = dict(window=c["shape"][0], group=c["shape"][1], words=c["cfg"][0], rounds=c["cfg"][1], floor=12)
    elif "blocktwins" in c:                                                # (the text of the narrow dealing cases)
        lst, T, SA = twin_list(c["blocktwins"], 1025 * 768 // 2, 3)
        args = dict(window=c["shape"][0], group=c["shape"][1], words=c["cfg"][0], rounds=c["cfg"][1], floor=12)
    else:
        nb, bl = c["blocks"]
        T, SA = _block_sa(nb, bl, 5)
        isa = inverse(SA)
        offs = np.array(list(range(300, 316)) + list(range(230, 238)) + list(range(0, 8)), np.int64)
        s1 = (np.arange(nb)[:, None] * bl + offs[None, :]).ravel()
        s2 = (nb * bl + (nb - 1 - np.arange(nb))[:, None] * bl + offs[None, :]).ravel()
        assert (np.abs(isa[s1] - isa[s2]) == 1).all()
        lo = np.sort(np.minimum(isa[s1], isa[s2]))
        lst = build_list(T, SA, lo, lo + 2, np.full(len(lo), 13, np.int64), 3)
        args = dict(window=c["shape"][0], group=c["shape"][1], words=c["cfg"][0], rounds=c["cfg"][1], floor=12)
    args.update(c["drv"])
    return dict(T=T, SA=SA, S=lst[0], P=lst[1], H=lst[2], C=lst[3], args=args)
