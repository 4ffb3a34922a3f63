"""Model of the suffix sorter's ranking step (k_rerank_reduce / k_rerank_scan_tiles / k_rerank_apply of
bwtc_amd/csrc/bwt_engine.hip, through launch_rerank), of the rounds' key kernels (k_gather_key2, k_gather_text,
k_gather_dense) and of the window scatters, in numpy and Python integers; and the named cases of tests/test_rankmodel.py
(no GPU) and tests/test_gpu_rank_step.py.

Inputs are honest: a case builds T, its suffix array comes from finmodel.suffix_array (prefix doubling, held to sorted()
by the CPU test), and a list is that suffix array under a key the case makes from the text -- the first k characters as
a base-sigma number, zero padded (the lowest symbol has code 0, so a suffix no longer than the key shares its key with
longer ones), as u32 or u64, with the suffix number's upper bits at bit 48 (split), or as long items: a key word, a
second word and one depth for all (the gram form), the same with made-up levels, or codemodel.py's keys (the code
form).  A round's list is what the model's own previous step left, sorted by (group, rank[s + h] + 1).  expect_round
restates the driver, rank_step once: the route from the counts, rank[] afterwards, the next list sorted by its keys.

The expectation restates the definition in the comment above rr_masks / k_rerank_apply, not the ballots:

  head[p]    p starts a group: p = 0, or the order key (key & kmask[, w & wmask]) differs from p - 1's, or (initial
             ranking) suffix p - 1 is no longer than the characters its key covers -- it is a proper prefix of everything
             that shares its key, a finished singleton.
  active[p]  p's group has two members or more.
  new rank   the global slot of the group's head (initial ranking: its list position; rounds: aglob of it).
  counts     active members, active groups.
  next list  the active members in list order: suffix, slot, dense group number (MODE 3: the new rank), character.
  stores     MODE 0 rank[s] = nr; 1 the pairs (s, nr); 2 records s << 32 | nr, values (group or all ones), plane
             (s >> rec_shift) & 255; 3 nothing.  A finished suffix: SA[slot] = s and, when the form emits, its character
             to out[slot] (slot out_n: last_char), pidx for suffix 0, lf[(n - s) / x] where x divides n - s and the
             quotient is in [1, lf_n).
  character  emit 1: bits 56..63 of the key; 2: T[s - 1] (0 for suffix 0); 3: inv_lut[the key's code field].
  aggregates as apply reads them: per tile of 2048 slots the exclusive sums of active members and active heads, and the
             exclusive max of "last head slot + 1".

Everything is deterministic and compared exactly.  Two properties come from the true suffix array alone (placed_breaks,
refined_breaks)."""
import functools

import numpy as np

import finmodel

suffix_array = finmodel.suffix_array          # shared, not copied

U64 = np.uint64
TILE, CHUNK, WAVE = 2048, 512, 64
SCAN_CHUNK = 4096
WIN_TILE = 2048
P32, P8, P16, P64 = 0xA5A5A5A5, 0xA5, 0xA5A5, 0xA5A5A5A5A5A5A5A5
LEVEL_DEPTH = (1, 8, 12, 16, 20, 24, 32, 48)  # code_level_depth


def rank_bits(n):
    """Bits of a round's second key: rank + 1 in 0 .. n (bwt_engine.hip, rank_bits)."""
    return max(1, (int(n) + 1).bit_length())


# ---- lists -------------------------------------------------------------------------------------------------------------
def dense_codes(T):
    """byte -> dense code in byte order (the lowest symbol of T gets 0, the padding's code), and sigma."""
    present = np.flatnonzero(np.bincount(np.asarray(T, np.uint8), minlength=256))
    lut = np.zeros(256, np.int64)
    lut[present] = np.arange(present.size)
    return lut, int(present.size)


def sigma_number(T, lut, sigma, at, k):
    """Characters T[at .. at + k) of every start in `at` as a base-sigma number, zero padded past the end (Python-exact:
    sigma ** k <= 2 ** 64 is the caller's)."""
    n = len(T)
    code = np.concatenate((lut[np.asarray(T, np.uint8)], np.zeros(k + 1, np.int64))).astype(U64)
    at = np.asarray(at, np.int64)
    v = np.zeros(at.size, U64)
    for j in range(k):
        v = v * U64(sigma) + code[np.minimum(at + j, n)]
    return v


def list_sigma(T, SA, k, wide=True, split=False, payload_seed=None):
    """The suffix array under the first k characters as a base-sigma number.  payload_seed: random bits above the key's
    (kmask then covers the key alone)."""
    T = np.asarray(T, np.uint8)
    n = T.size
    lut, sigma = dense_codes(T)
    bits = max(1, int(sigma ** k - 1).bit_length())
    assert bits <= (48 if split else 64 if wide else 32)
    sfx = np.asarray(SA, np.int64)
    keys = sigma_number(T, lut, sigma, sfx, k)
    width = 64 if wide else 32
    kmask = (1 << width) - 1
    if split:
        keys = keys | ((sfx >> 16).astype(U64) << U64(48))
        kmask = (1 << 48) - 1
    elif payload_seed is not None and bits < width:
        rng = np.random.default_rng(payload_seed)
        keys = keys | (rng.integers(0, 1 << (width - bits), n, dtype=np.uint64) << U64(bits))
        kmask = (1 << bits) - 1
    return dict(n=n, m=n, init=True, wide=wide, split=split, keys=keys if wide else keys.astype(np.uint32), sfx=sfx, kmask=kmask, short_len=k,
                depth=np.full(n, k, np.int64), w=None, aglob=None, long=None, inv_lut=None, claim=k)


def list_gram(T, SA, k1, k2, wbits, split=False, garbage_seed=5):
    """Long items of the gram form: the key word holds k1 characters, the second word the next k2 in its low wbits bits
    (random bits above them, which wmask hides), every item shares depth k1 + k2; the predecessor's code rides at chr_shift
    and inv_lut (no identity) turns it back."""
    T = np.asarray(T, np.uint8)
    n = T.size
    lut, sigma = dense_codes(T)
    key_bits = max(1, int(sigma ** k1 - 1).bit_length())
    assert int(sigma ** k2 - 1).bit_length() <= wbits <= 32
    cb = max(1, int(sigma - 1).bit_length())
    hi_shift, chr_shift = key_bits, key_bits + (13 if split else 0)
    assert chr_shift + cb <= 64
    sfx = np.asarray(SA, np.int64)
    keys = sigma_number(T, lut, sigma, sfx, k1)
    w = sigma_number(T, lut, sigma, sfx + k1, k2)
    prev = np.where(sfx > 0, lut[T[np.maximum(sfx - 1, 0)]], 0).astype(U64)
    keys = keys | (prev << U64(chr_shift))
    if split:
        keys = keys | ((sfx >> 16).astype(U64) << U64(hi_shift))
    rng = np.random.default_rng(garbage_seed)
    if wbits < 32:
        w = w | (rng.integers(0, 1 << (32 - wbits), n, dtype=np.uint64) << U64(wbits))
    inv = np.zeros(256, np.uint8)
    inv[lut[np.flatnonzero(np.bincount(T, minlength=256))]] = np.flatnonzero(np.bincount(T, minlength=256))
    long = dict(wmask=(1 << wbits) - 1, hi_shift=hi_shift, chr_shift=chr_shift, chr_mask=(1 << cb) - 1, lvl_shift=-1, depth=k1 + k2)
    return dict(n=n, m=n, init=True, wide=True, split=split, keys=keys, sfx=sfx, kmask=(1 << key_bits) - 1, short_len=k1 + k2,
                depth=np.full(n, k1 + k2, np.int64), w=w.astype(np.uint32), aglob=None, long=long, inv_lut=inv, claim=k1 + k2)


def with_levels(L, levels, lvl_shift):
    """A gram-form long list given per-item levels at lvl_shift instead of one depth (the code form's field): the items of
    a group share a level, as a code key's do -- `levels` is indexed by the group's first k1 characters' number."""
    keys = L["keys"].copy()
    lv = np.asarray(levels, np.int64)[(keys & U64(L["kmask"])).astype(np.int64) % len(levels)]
    keys = keys | (lv.astype(U64) << U64(lvl_shift))
    M = dict(L, keys=keys, long=dict(L["long"], lvl_shift=lvl_shift), depth=np.array(LEVEL_DEPTH, np.int64)[lv], short_len=0, claim=None)
    return M


def device_idx(L):
    """idx as the hook takes it: suffix numbers, or with split their 16-bit lower halves."""
    return (L["sfx"] & 0xFFFF).astype(np.uint16) if L["split"] else L["sfx"].astype(np.uint32)


# ---- the step ----------------------------------------------------------------------------------------------------------
def _chars(T, L, emit):
    s, keys = L["sfx"], L["keys"].astype(U64)
    if emit == 1:
        return (keys >> U64(56)).astype(np.int64)
    if emit == 2:
        return np.where(s > 0, np.asarray(T, np.uint8)[np.maximum(s - 1, 0)], 0).astype(np.int64)
    if emit == 3:
        lg = L["long"]
        return L["inv_lut"][((keys >> U64(lg["chr_shift"])).astype(np.int64) & lg["chr_mask"]) & 0xFF].astype(np.int64)
    return np.zeros(len(s), np.int64)


def structure(L):
    """head, size of the group (per member), position of the group's head, active -- from the definition."""
    m, n = L["m"], L["n"]
    kc = L["keys"].astype(U64) & U64(L["kmask"])
    head = np.ones(m, bool)
    head[1:] = kc[1:] != kc[:-1]
    if L["w"] is not None:
        wc = L["w"].astype(np.int64) & L["long"]["wmask"]
        head[1:] |= wc[1:] != wc[:-1]
    if L["init"]:
        head[1:] |= (n - L["sfx"][:-1]) <= L["depth"][:-1]              # p - 1 is no longer than its key: a finished singleton
    first = np.maximum.accumulate(np.where(head, np.arange(m), 0))
    gid = np.cumsum(head) - 1
    size = np.bincount(gid)[gid]
    return head, size, first, size >= 2


def expect_pass(T, L, mode=0, emit=0, out_n=None, lf_n=0, rec_shift=0, plane=True):
    T = np.asarray(T, np.uint8)
    n, m = L["n"], L["m"]
    out_n = n if out_n is None else out_n
    head, size, first, act = structure(L)
    s = L["sfx"]
    g = np.arange(m) if L["init"] else L["aglob"].astype(np.int64)
    nr = g[first]
    c = _chars(T, L, emit)
    ah = act & head
    grp = np.cumsum(ah) - 1
    tiles = -(-m // TILE)
    tid = np.arange(m) // TILE
    per_a = np.bincount(tid, weights=act, minlength=tiles).astype(np.int64)
    per_b = np.bincount(tid, weights=ah, minlength=tiles).astype(np.int64)
    last = np.zeros(tiles, np.int64)
    np.maximum.at(last, tid[head], np.flatnonzero(head) + 1)
    res = dict(aggA=(np.cumsum(per_a) - per_a).astype(np.uint32), aggB=(np.cumsum(per_b) - per_b).astype(np.uint32),
               aggC=np.concatenate(([0], np.maximum.accumulate(last)[:-1])).astype(np.uint32),
               counts=np.array([act.sum(), ah.sum()], np.uint32))
    res.update(rank=np.full(n, P32, np.uint32), pair_s=np.full(m, P32, np.uint32), pair_r=np.full(m, P32, np.uint32), rec=np.full(m, P64, U64),
               val=np.full(m, P32, np.uint32), rplane=np.full(m, P8, np.uint8), aidx=np.full(m, P32, np.uint32), aglob=np.full(m, P32, np.uint32),
               agrp=np.full(m, P32, np.uint32), achr=np.full(m, P16 if mode == 3 else P8, np.uint16 if mode == 3 else np.uint8),
               SA=np.full(n, P32, np.uint32), out=np.full(n, P8, np.uint8), pidx=P32, last_char=P32, lf=np.full(256, P32, np.uint32))
    if mode == 0:
        res["rank"][s] = nr
    elif mode == 1:
        res["pair_s"][:], res["pair_r"][:] = s, nr
    elif mode == 2:
        res["rec"][:] = (s.astype(U64) << U64(32)) | nr.astype(U64)
        res["val"][:] = np.where(act, grp, 0xFFFFFFFF)
        if plane:
            res["rplane"][:] = (s >> rec_shift) & 255
    q = int(act.sum())
    res["aglob"][:q] = g[act]
    if mode != 2:
        res["aidx"][:q] = s[act]
        res["agrp"][:q] = nr[act] if mode == 3 else grp[act]
        if mode == 3:
            dlow = (L["depth"] & 0xFF) << 8 if L["long"] is not None else 0
            res["achr"][:q] = ((c & 0xFFFF) | dlow)[act] if L["long"] is not None else (c & 0xFFFF)[act]
        elif emit:
            res["achr"][:q] = c[act] & 0xFF
    fin = ~act
    res["SA"][g[fin]] = s[fin]
    if emit:
        fg, fs, fc = g[fin], s[fin], c[fin]
        inside = fg < out_n
        res["out"][fg[inside]] = fc[inside] & 0xFF
        if (~inside).any():
            res["last_char"] = int(fc[~inside][-1])
        if (fs == 0).any():
            res["pidx"] = int(fg[fs == 0][0])
        if lf_n > 1:
            x = n // lf_n
            t = n - fs
            hit = (t % x == 0) & (t // x >= 1) & (t // x < lf_n)
            res["lf"][(t // x)[hit]] = fg[hit]
    res.update(_head=head, _act=act, _nr=nr, _size=size, _g=g, _first=first, _depth=L["depth"][act])
    return res


def slow_pass(T, L, mode=0, emit=0, out_n=None, lf_n=0, rec_shift=0, plane=True):
    """The same, slot by slot in plain Python."""
    n, m = L["n"], L["m"]
    out_n = n if out_n is None else out_n
    keys, s = [int(v) for v in L["keys"]], [int(v) for v in L["sfx"]]
    w = [int(v) & L["long"]["wmask"] for v in L["w"]] if L["w"] is not None else [0] * m
    depth = [int(v) for v in L["depth"]]
    g = list(range(m)) if L["init"] else [int(v) for v in L["aglob"]]
    head = []
    for p in range(m):
        h = p == 0 or (keys[p] & L["kmask"], w[p]) != (keys[p - 1] & L["kmask"], w[p - 1])
        if L["init"] and p > 0 and n - s[p - 1] <= depth[p - 1]:
            h = True
        head.append(h)
    tiles = -(-m // TILE)
    A, B, C = [0] * tiles, [0] * tiles, [0] * tiles
    o = dict(rank=[P32] * n, pair_s=[P32] * m, pair_r=[P32] * m, rec=[P64] * m, val=[P32] * m, rplane=[P8] * m, aidx=[P32] * m, aglob=[P32] * m,
             agrp=[P32] * m, achr=[P16 if mode == 3 else P8] * m, SA=[P32] * n, out=[P8] * n, pidx=P32, last_char=P32, lf=[P32] * 256)
    q = ngrp = 0
    a_seen = b_seen = c_seen = 0
    p = 0
    while p < m:
        e = p + 1
        while e < m and not head[e]:
            e += 1
        active = e - p >= 2
        for j in range(p, e):
            if j % TILE == 0:
                A[j // TILE], B[j // TILE], C[j // TILE] = a_seen, b_seen, c_seen
            if j == p:
                c_seen = p + 1
                b_seen += active
            a_seen += active
            nr = g[p]
            if emit == 1:
                ch = keys[j] >> 56
            elif emit == 2:
                ch = int(T[s[j] - 1]) if s[j] else 0
            elif emit == 3:
                ch = int(L["inv_lut"][((keys[j] >> L["long"]["chr_shift"]) & L["long"]["chr_mask"]) & 0xFF])
            else:
                ch = 0
            if mode == 0:
                o["rank"][s[j]] = nr
            elif mode == 1:
                o["pair_s"][j], o["pair_r"][j] = s[j], nr
            elif mode == 2:
                o["rec"][j], o["val"][j] = (s[j] << 32) | nr, ngrp if active else 0xFFFFFFFF
                if plane:
                    o["rplane"][j] = (s[j] >> rec_shift) & 255
            if active:
                o["aglob"][q] = g[j]
                if mode != 2:
                    o["aidx"][q] = s[j]
                    o["agrp"][q] = nr if mode == 3 else ngrp
                    if mode == 3:
                        o["achr"][q] = ch | (((depth[j] & 0xFF) << 8) if L["long"] is not None else 0)
                    elif emit:
                        o["achr"][q] = ch & 0xFF
                q += 1
            else:
                o["SA"][g[j]] = s[j]
                if emit:
                    if s[j] == 0:
                        o["pidx"] = g[j]
                    if g[j] < out_n:
                        o["out"][g[j]] = ch & 0xFF
                    else:
                        o["last_char"] = ch
                    if lf_n > 1:
                        x, t = n // lf_n, n - s[j]
                        if t % x == 0 and 1 <= t // x < lf_n:
                            o["lf"][t // x] = g[j]
        ngrp += active
        p = e
    o.update(aggA=A, aggB=B, aggC=C, counts=[q, ngrp])
    return o


FIELDS = ("aggA", "aggB", "aggC", "counts", "rank", "aglob", "rplane", "SA", "out", "pidx", "last_char", "lf")


def compared(mode):
    return FIELDS + (("rec", "val") if mode == 2 else ("pair_s", "pair_r", "aidx", "agrp", "achr"))


def differences(want, have, mode):
    """Names of the outputs in which a result differs from the expectation."""
    bad = []
    for f in compared(mode):
        a, b = want[f], have[f]
        same = int(a) == int(b) if np.isscalar(a) or isinstance(a, int) else (len(a) == len(b) and bool((np.asarray(a, np.uint64) == np.asarray(b, np.uint64)).all()))
        if not same:
            bad.append(f)
    return bad


# ---- the two properties, from the true suffix array alone -------------------------------------------------------------
def placed_breaks(T, SA_true, res, emit, out_n=None):
    """Finished (slot, s) with s != SA[slot], or whose byte is not T[s - 1] (slot out_n: last_char; suffix 0: pidx alone).  The byte
    is asked of the forms that read or decode it (2, 3); form 1 hands on what the key carried."""
    T = np.asarray(T, np.uint8)
    n = len(T)
    out_n = n if out_n is None else out_n
    SA, out = np.asarray(res["SA"]), np.asarray(res["out"])
    slots = np.flatnonzero(SA != P32)
    bad = int((SA[slots] != SA_true[slots]).sum())
    if emit in (2, 3):
        s = SA[slots].astype(np.int64)
        byte = np.where(s > 0, T[np.maximum(s - 1, 0)], 0)
        ins = (slots < out_n) & (s > 0)                    # (the row of suffix 0 is the end-of-block row: k_finalize writes its byte)
        bad += int((out[slots[ins]] != byte[ins]).sum())
        last = (slots >= out_n) & (s > 0)
        if last.any():
            bad += int(res["last_char"] != int(byte[last][0]))
        z = slots[s == 0]
        bad += int(len(z) > 0 and res["pidx"] != int(z[0]))
        bad += int((out[np.setdiff1d(np.arange(n), slots)] != P8).sum())
    return bad


def refined_breaks(T, SA_true, slots, sfx, ranks, depth):
    """Groups left -- given as the members' slots, suffixes and new ranks -- that are not a slot range of SA, whose rank is
    not their head's slot, whose members do not share `depth` characters (zero padded; None: not asked), or that have one
    member."""
    T = np.asarray(T, np.uint8)
    n = len(T)
    slots, sfx, ranks = (np.asarray(a, np.int64) for a in (slots, sfx, ranks))
    if not len(slots):
        return 0
    bad = int((np.diff(slots) <= 0).sum())
    new = np.ones(len(slots), bool)
    new[1:] = ranks[1:] != ranks[:-1]
    first = np.maximum.accumulate(np.where(new, np.arange(len(slots)), 0))
    bad += int((slots != ranks + np.arange(len(slots)) - first).sum())     # a range that begins at its rank
    bad += int((np.bincount(np.cumsum(new) - 1) < 2).sum())
    gid = np.cumsum(new)
    a = np.lexsort((sfx, gid))
    b = np.lexsort((SA_true[np.minimum(slots, n - 1)].astype(np.int64), gid))
    bad += int((sfx[a] != SA_true[np.minimum(slots, n - 1)].astype(np.int64)[b]).sum())
    if depth is not None:
        d = np.broadcast_to(np.asarray(depth, np.int64), sfx.shape)
        Tp = finmodel.padded(T, 8)
        lead = sfx[first]
        for j in range(int(d.max())):
            bad += int(((Tp[np.minimum(sfx + j, n)] != Tp[np.minimum(lead + j, n)]) & (j < d)).sum())
    return bad


def left_of(res, mode):
    """The groups a step left, as refined_breaks takes them: (slots, suffixes, ranks)."""
    q = int(res["counts"][0])
    if mode == 2:
        rec, val = np.asarray(res["rec"], U64), np.asarray(res["val"])
        a = val != 0xFFFFFFFF
        return np.asarray(res["aglob"])[:q], (rec[a] >> U64(32)).astype(np.int64), (rec[a] & U64(0xFFFFFFFF)).astype(np.int64)
    if mode == 3:
        return np.asarray(res["aglob"])[:q], np.asarray(res["aidx"])[:q], np.asarray(res["agrp"])[:q]
    aglob, agrp = np.asarray(res["aglob"], np.int64)[:q], np.asarray(res["agrp"], np.int64)[:q]
    new = np.ones(q, bool)
    new[1:] = agrp[1:] != agrp[:-1]
    first = np.maximum.accumulate(np.where(new, np.arange(q), 0)) if q else np.zeros(0, np.int64)
    return aglob, np.asarray(res["aidx"])[:q], aglob[first]


# ---- the scan ----------------------------------------------------------------------------------------------------------
def expect_scan(a, b, c):
    """Exclusive sums of a and b modulo 2^32, exclusive max of c; the parts per 4096 entries; the totals."""
    a, b, c = (np.asarray(x, np.uint64) for x in (a, b, c))
    nt = a.size
    ea = (np.cumsum(a) - a) & U64(0xFFFFFFFF)
    eb = (np.cumsum(b) - b) & U64(0xFFFFFFFF)
    ec = np.concatenate(([0], np.maximum.accumulate(c)[:-1])).astype(np.uint64)
    parts = []
    for lo in range(0, nt, SCAN_CHUNK):
        parts += [int(a[lo:lo + SCAN_CHUNK].sum()) & 0xFFFFFFFF, int(b[lo:lo + SCAN_CHUNK].sum()) & 0xFFFFFFFF, int(c[lo:lo + SCAN_CHUNK].max())]
    counts = [int(a.sum()) & 0xFFFFFFFF, int(b.sum()) & 0xFFFFFFFF]
    return ea.astype(np.uint32), eb.astype(np.uint32), ec.astype(np.uint32), np.array(parts, np.uint32), np.array(counts, np.uint32)


# ---- the rounds' keys --------------------------------------------------------------------------------------------------
def run_key2(T, rank, k, s, n, h, b2, run_mode, h_split, p):
    """The second key of suffix s (Python integers): the comment above RunKeys / run_key2, restated."""
    if run_mode == 1 and int(k[s]) >= h:
        kk = int(k[s])
        e = s + kk
        falling = e >= n or T[e] < T[e - p]
        return kk if falling else (1 << (b2 - 1)) | (n - kk)
    if rank is None:
        return 0
    off = h
    if run_mode == 2 and int(k[s]) >= h_split:
        off = max(h, int(k[s]))
    t = s + off
    return int(rank[t]) + 1 if t < n else 0


def expect_key2(T, aidx, agrp, rank, achr, h, b2, run_mode=0, k=None, h_split=0, p=1):
    n = len(T)
    out = []
    for i in range(len(aidx)):
        s = int(aidx[i])
        v = (int(agrp[i]) << b2) | run_key2(T, rank, k, s, n, h, b2, run_mode, h_split, p)
        out.append((v | ((int(achr[i]) << 56) if achr is not None else 0)) & (2 ** 64 - 1))
    return np.array(out, U64)


def expect_text(T, aidx, agrp, achr, h, c, run_mode=0, k=None, h_split=0):
    """group << (8 c + 4) | the next c characters << 4 | c - (characters past the end)."""
    n = len(T)
    out = []
    for i in range(len(aidx)):
        s = int(aidx[i])
        at = s + h
        if run_mode == 2 and int(k[s]) >= h_split:
            at = s + int(k[s]) + (h - h_split)
        chars = 0
        for j in range(c):
            chars = (chars << 8) | (int(T[at + j]) if at + j < n else 0)
        over = min(c, max(0, at + c - n))
        v = (int(agrp[i]) << (8 * c + 4)) | (chars << 4) | (c - over)
        out.append(v | ((int(achr[i]) << 56) if achr is not None else 0))
    return np.array(out, U64)


def expect_dense(T, rec, val, rank, h, b2, emit, run_mode=0, k=None, h_split=0, p=1):
    """Per record (key, value): the order inside a chunk of 2048 is free, so chunk_multisets() compares."""
    n = len(T)
    keys, vals = [], []
    for i in range(len(rec)):
        s, g = int(rec[i]) >> 32, int(val[i])
        key = 2 ** 64 - 1
        if g != 0xFFFFFFFF:
            c = int(T[s - 1]) if (emit and s) else 0
            key = (g << b2) | run_key2(T, rank, k, s, n, h, b2, run_mode, h_split, p) | (c << 56)
        keys.append(key)
        vals.append(s)
    return np.array(keys, U64), np.array(vals, np.uint32)


def chunk_multisets(keys, vals):
    """(key, value) pairs sorted inside every chunk of 2048."""
    keys, vals = np.asarray(keys, U64), np.asarray(vals, np.uint32)
    out_k, out_v = keys.copy(), vals.copy()
    for lo in range(0, len(keys), WIN_TILE):
        o = np.lexsort((vals[lo:lo + WIN_TILE], keys[lo:lo + WIN_TILE]))
        out_k[lo:lo + WIN_TILE], out_v[lo:lo + WIN_TILE] = keys[lo:lo + WIN_TILE][o], vals[lo:lo + WIN_TILE][o]
    return out_k, out_v


def next_round(T, L, res, rank, h, carry, key2=None):
    """The list the next round ranks: the active members of `res` (a MODE 0 or 1 step over L) sorted by (group,
    rank[s + h] + 1), their slots staying in place; carry: the character in bits 56..63 (kmask hides it)."""
    n = L["n"]
    q = int(res["counts"][0])
    aidx, agrp, aglob = (np.asarray(res[f], np.int64)[:q] for f in ("aidx", "agrp", "aglob"))
    b2 = rank_bits(n)
    achr = np.asarray(res["achr"])[:q] if carry else None
    keys = (key2 or (lambda *a: expect_key2(T, *a)))(aidx, agrp, rank, achr, h, b2)     # key2: the device's k_gather_key2 instead
    order = np.argsort(keys & U64((1 << 56) - 1) if carry else keys, kind="stable")
    return dict(n=n, m=q, init=False, wide=True, split=False, keys=keys[order], sfx=aidx[order], kmask=(1 << 56) - 1 if carry else 2 ** 64 - 1,
                short_len=0, depth=np.zeros(q, np.int64), w=None, aglob=aglob, long=None, inv_lut=None, claim=None)


def chain(T, L0, emit_first=2, step=None, out_n=None, lf_n=0, key2=None):
    """The initial ranking of L0 and every doubling round until nothing is active, through `step` (default: the model) ->
    (SA, out, pidx, last_char, lf, rounds).  rank[] is kept as the steps leave it (MODE 0)."""
    n = L0["n"]
    step = step or (lambda L, emit: expect_pass(T, L, 0, emit, out_n, lf_n))
    SA, out, lf = np.full(n, P32, np.uint32), np.full(n, P8, np.uint8), np.full(256, P32, np.uint32)
    pidx = last_char = P32
    rank = np.full(n, P32, np.uint32)
    L, emit, h, rounds = L0, emit_first, L0["short_len"], 0
    while True:
        res = step(L, emit)
        touched = np.asarray(res["rank"]) != P32
        rank[touched] = np.asarray(res["rank"])[touched]
        fin = np.asarray(res["SA"]) != P32
        SA[fin] = np.asarray(res["SA"])[fin]
        o = np.asarray(res["out"])
        if emit:
            out[fin] = o[fin]
        pidx = res["pidx"] if res["pidx"] != P32 else pidx
        last_char = res["last_char"] if res["last_char"] != P32 else last_char
        l = np.asarray(res["lf"])
        lf[l != P32] = l[l != P32]
        if int(res["counts"][0]) == 0 or rounds > 40:
            return SA, out, pidx, last_char, lf, rounds
        carry = emit != 0
        L = next_round(T, L, res, rank, h, carry, key2)
        emit = 1 if carry else 0
        h *= 2
        rounds += 1


def expect_round(T, L, rank, h_next, emit=False, text=False, carry_in=False, raw_out=False, run_mode=0, k=None, step_p=1, step_depth=0,
                 pairs_min=1 << 21, out_n=None, lf_n=0):
    """rank_step<u64, false> once over the round list L, restated: the route from the counts (raw; text; dense when at
    least half of a list of pairs_min entries stays active; pairs for a list that long; short), the step itself, rank[]
    afterwards, and the next list sorted by its keys -- stably, but for the dense route, where the order among equal keys
    is free.  -> dict: route, m, groups, carry, text_chars, ran_run, ks, vs, aglob, rank, stable, and the step's emissions."""
    n, m = L["n"], L["m"]
    form = 0 if not emit else (1 if carry_in else 2)
    probe = expect_pass(T, L, 3, form, out_n, lf_n)
    q, groups = int(probe["counts"][0]), int(probe["counts"][1])
    b2, b1 = rank_bits(n), max(0, groups - 1).bit_length()
    run_now = run_mode == 1
    b2k, kbits = (b2 + 1, b1 + b2 + 1) if run_now else (b2, b1 + b2)
    carry_next = bool(emit) and kbits <= 56
    dense = (not text) and q > 0 and 2 * q >= m and m >= pairs_min
    route = "raw" if raw_out else "text" if text else "dense" if dense else "pairs" if m >= pairs_min else "short"
    mode = dict(raw=3, text=0, dense=2, pairs=1, short=0)[route]
    res = expect_pass(T, L, mode, form, out_n, lf_n)
    rank_after = np.array(rank, np.uint32)
    if route != "raw":
        rank_after[L["sfx"]] = res["_nr"]
    out = dict(route=route, m=q, groups=groups, ran_run=run_now, rank=rank_after, aglob=res["aglob"][:q] if route != "raw" else res["aglob"],
               stable=route != "dense", step=res, text_chars=0, carry=carry_next)
    if route == "raw":
        out.update(carry=bool(emit), vs=res["aidx"][:q], grp=res["agrp"][:q], chr=res["achr"][:q])
        return out
    act = res["_act"]
    aidx, grp = L["sfx"][act], (np.cumsum(act & res["_head"]) - 1)[act]
    c = _chars(T, L, form)[act] & 0xFF
    if text and (q == 0 or not run_now):
        tc = min(6, (56 - b1 - 4) // 8)
        out.update(carry=bool(emit), text_chars=tc)
        keys = expect_text(T, aidx, grp, c if emit else None, h_next, tc, 2 if run_mode == 2 else 0, k, step_depth)
        bits = b1 + 8 * tc + 4
    else:
        if text:
            out["text_chars"] = 0
        rk = None if text else rank_after
        keys = expect_key2(T, aidx, grp, rk, c if carry_next else None, min(h_next, 0xFFFFFFFF), b2k, 1 if run_now else (2 if run_mode == 2 else 0), k,
                           0 if run_now else step_depth, step_p)
        bits = kbits
    if q == 0:
        out.update(ks=keys[:0], vs=aidx[:0].astype(np.uint32), text_chars=out["text_chars"] if text else 0)
        return out
    order = np.argsort(keys & U64((1 << bits) - 1), kind="stable")
    out.update(ks=keys[order], vs=aidx[order].astype(np.uint32))
    return out


def stretch_lengths(T, p):
    """k_p[s]: the leading characters of suffix s that are p-periodic (p = 1: the run from s on), by definition."""
    T = np.asarray(T, np.uint8)
    n = len(T)
    brk = np.zeros(n + 1, bool)
    brk[n] = True
    brk[p:n] = T[p:] != T[:n - p]
    nxt = np.full(n + 2, n, np.int64)
    for q in range(n, -1, -1):
        nxt[q] = q if brk[q] else nxt[q + 1]
    s = np.arange(n)
    return (nxt[np.minimum(s + p, n)] - s).astype(np.uint32)


def runs_heavy_text(n, seed):
    """Runs of 1 .. 40 copies of three symbols, ending in the lowest."""
    rng = np.random.default_rng(seed)
    parts, total = [], 0
    while total < n:
        parts.append(np.full(int(rng.integers(1, 41)), int(rng.integers(1, 4)), np.uint8))
        total += len(parts[-1])
    T = np.concatenate(parts)[:n]
    T[n - 3:] = 1
    return T


def driver_cases():
    """name -> dict(T, k, the flags of the call, pairs_min as a function of the list's size, the route it must take)."""
    rnd, small, phr, runs = random_text(16000, 4, 31, tail=2), random_text(4096, 4, 32, tail=2), form_text(16000, 8), runs_heavy_text(12000, 6)
    return dict(
        short=dict(T=rnd, k=4, pm=lambda m: m + 1, route="short"),
        pairs_sorted=dict(T=rnd, k=4, pm=lambda m: m, route="pairs"),
        pairs_unsorted=dict(T=small, k=4, pm=lambda m: m, route="pairs"),            # n - 1 has 12 bits: no partition sort
        dense=dict(T=phr, k=4, pm=lambda m: m, route="dense"),
        dense_no_emit=dict(T=phr, k=4, pm=lambda m: m, route="dense", emit=False),
        text=dict(T=phr, k=4, pm=lambda m: m, route="text", text=True),
        text_run=dict(T=runs, k=4, pm=lambda m: m + 1, route="text", text=True, run_mode=1, same_h=True),
        short_after_run=dict(T=runs, k=4, pm=lambda m: m + 1, route="short", run_mode=2, step_depth=4),
        raw=dict(T=phr, k=4, pm=lambda m: m, route="raw", text=True, raw_out=True))


def make_driver(c):
    """-> (T, list, rank[], the keyword arguments of expect_round / Context.test_round but pairs_min and window_bits)."""
    T = c["T"]
    emit = c.get("emit", True)
    L, rank, h = round_list(T, c["k"], emit)
    kw = dict(h_next=h if c.get("same_h") else 2 * h, emit=emit, text=c.get("text", False), carry_in=emit, raw_out=c.get("raw_out", False),
              run_mode=c.get("run_mode", 0), step_p=1, step_depth=c.get("step_depth", 0), out_n=len(T) - 1, lf_n=5)
    if kw["run_mode"]:
        kw["k"] = stretch_lengths(T, 1)
    return T, L, rank, kw


def canon_pairs(ks, vs):
    """(key, value) sorted by both: what is pinned where the order among equal keys is free."""
    o = np.lexsort((np.asarray(vs), np.asarray(ks, U64)))
    return np.asarray(ks, U64)[o], np.asarray(vs)[o]


def round_differences(want, have):
    bad = [f for f in ("m", "groups", "carry", "text_chars", "ran_run") if int(want[f]) != int(have[f])]
    st = want["step"]
    if want["route"] == "raw":
        bad += [f for f in ("vs", "grp", "chr") if not np.array_equal(np.asarray(want[f], np.uint64), np.asarray(have[f], np.uint64)[:want["m"]])]
        bad += ["aglob"] if not np.array_equal(want["aglob"], have["aglob"]) else []
    else:
        a, b = ((want["ks"], want["vs"]), (have["ks"], have["vs"])) if want["stable"] else (canon_pairs(want["ks"], want["vs"]), canon_pairs(have["ks"], have["vs"]))
        bad += ["ks"] if not np.array_equal(a[0], b[0]) else []
        bad += ["vs"] if not np.array_equal(a[1], b[1]) else []
        bad += ["aglob"] if not np.array_equal(want["aglob"], have["aglob"][:want["m"]]) or (have["aglob"][want["m"]:] != P32).any() else []
    bad += [f for f in ("rank",) if not np.array_equal(want[f], have[f])]
    bad += [f for f in ("SA", "out", "lf") if not np.array_equal(np.asarray(st[f], np.uint64), np.asarray(have[f], np.uint64))]
    bad += [f for f in ("pidx", "last_char") if int(st[f]) != int(have[f])]
    return bad


def round_left(have, raw):
    """The groups a driver step left, as refined_breaks takes them: slots ascending, the members by their new rank."""
    if raw:
        q = have["m"]
        return have["aglob"][:q], have["vs"][:q], have["grp"][:q]
    r = np.asarray(have["rank"], np.int64)[np.asarray(have["vs"], np.int64)]
    o = np.argsort(r, kind="stable")
    return have["aglob"][:have["m"]], np.asarray(have["vs"])[o], r[o]


# ---- texts and cases ---------------------------------------------------------------------------------------------------
def runs_text(lengths, tail=0, first=1):
    """Runs of ascending bytes first, first + 1, ... with the given lengths, then `tail` copies of the lowest byte: under a
    key of k characters run i's suffixes take the slots [sum of the lengths before it + tail, ...) -- a group of length - k
    + 1 members, then k - 1 singletons -- and the tail's suffixes, no longer than the key or just longer, take the first."""
    assert len(lengths) + first <= 256
    parts = [np.full(int(l), first + i, np.uint8) for i, l in enumerate(lengths)]
    return np.concatenate(parts + [np.full(tail, first, np.uint8)])


def random_text(n, sigma, seed, tail=0):
    rng = np.random.default_rng(seed)
    T = rng.integers(0, sigma, n, dtype=np.uint8) + np.uint8(1)
    if tail:
        T[n - tail:] = 1
    return T


def phrase_text(n, seed, sigma=4, nphr=5, plen=40):
    """Random text with repeated phrases: groups that take several rounds."""
    rng = np.random.default_rng(seed)
    phr = [rng.integers(0, sigma, plen, dtype=np.uint8) + np.uint8(1) for _ in range(nphr)]
    parts, total = [], 0
    while total < n:
        x = phr[int(rng.integers(0, nphr))] if rng.random() < 0.6 else rng.integers(0, sigma, int(rng.integers(1, 9)), dtype=np.uint8) + np.uint8(1)
        parts.append(x)
        total += len(x)
    return np.concatenate(parts)[:n]


@functools.lru_cache(maxsize=None)
def _sa_cached(key):
    T = np.frombuffer(key, np.uint8)
    return suffix_array(T)


def sa_of(T):
    return _sa_cached(np.asarray(T, np.uint8).tobytes())


SIZES = (1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 3 * 2048 - 1, 3 * 2048, 3 * 2048 + 1, 17 * 2048 + 5)
GROUP_SIZES = (2, 64, 65, 512, 513, 2049, 2 * 2048 + 3)
SEAMS = dict(lane=2 * 2048 + 3 * 64, iteration=2 * 2048 + 512 + 64 * 4, chunk=2 * 2048 + 512, tile=2 * 2048)
# (lane: a multiple of 64 inside an iteration's row; iteration: where a wave goes on to its next row of 64 -- the same
# seam for the ballots, kept apart because the neighbour then comes from another register; chunk: a wave's 512 slots; tile)
K = 4


def seam_lengths(k, at, size):
    """Run lengths for runs_text that put a group of `size` members at slot `at`: one long run in front (a group from slot 0
    that crosses the tiles before `at`, then its k - 1 singletons), a hundred runs of one (singletons), the group's run, and
    a short last run (the last run's suffixes end the text and are laid out differently)."""
    lengths = [at - 100] + [1] * 100 if at > 200 else [1] * at
    return lengths + [size + k - 1, 2]


def pass_cases():
    """name -> dict(T, the list's kind and arguments, edge: what the case is named for).  tests/test_rankmodel.py holds every
    case to its edge, on the model's own head and group arrays."""
    cs = {}
    for m in SIZES:
        cs["size_%d" % m] = dict(T=random_text(m, 4, 100 + m, tail=min(m, 3)), kind="sigma", k=4 if m < 2047 else 8, edge=("m", m))
    for name, seam in SEAMS.items():
        for d in (-1, 0, 1):
            cs["start_%s_%+d" % (name, d)] = dict(T=runs_text(seam_lengths(K, seam + d, 70)), kind="sigma", k=K, edge=("start", seam + d, 70))
    for gs in GROUP_SIZES:
        cs["group_%d" % gs] = dict(T=runs_text(seam_lengths(K, 2047, gs)), kind="sigma", k=K, edge=("start", 2047, gs))
    cs["three_tiles"] = dict(T=runs_text(seam_lengths(K, 2040, 4 * 2048 + 10 - 2040)), kind="sigma", k=K, edge=("span3", 2040, 4 * 2048 + 10 - 2040))
    # 65 tiles and more: the scan's second row of 64 aggregates, with a head carried into it from tile 0
    cs["scan_row_65"] = dict(T=runs_text(seam_lengths(K, 65 * 2048 + 100, 70)), kind="sigma", k=K, edge=("start", 65 * 2048 + 100, 70))
    cs["head_last_slot"] = dict(T=runs_text(seam_lengths(K, 2 * 2048 - 1, 9)), kind="sigma", k=K, edge=("start", 2 * 2048 - 1, 9))
    cs["all_singletons"] = dict(T=np.random.default_rng(9).permutation(np.repeat(np.arange(1, 251, dtype=np.uint8), 20)), kind="sigma", k=6,
                                edge=("active_at_most", 40))
    cs["one_group"] = dict(T=runs_text([5000]), kind="sigma", k=1, edge=("groups", 1))
    cs["idle_tile"] = dict(T=np.concatenate((np.full(3000, 1, np.uint8), np.random.default_rng(3).integers(2, 202, 4200, dtype=np.uint8))),
                           kind="sigma", k=4, edge=("idle_tile",))
    # the short-suffix rule: texts ending in their lowest symbol; the tail's suffixes share the key of longer ones
    for k in (1, 4, 8):
        cs["short_%d" % k] = dict(T=runs_text([40, 9, 2100, 5], tail=k + 3), kind="sigma", k=k, edge=("short", k))
    cs["payload"] = dict(T=random_text(5000, 4, 77, tail=2), kind="sigma", k=5, payload=11, edge=("payload",))
    return cs


def make_list(c, **kw):
    T = c["T"]
    SA = sa_of(T)
    if c["kind"] == "sigma":
        return list_sigma(T, SA, c["k"], **dict(dict(wide=c.get("wide", True), split=c.get("split", False), payload_seed=c.get("payload")), **kw))
    return list_gram(T, SA, c["k1"], c["k2"], c["wbits"], split=c.get("split", False))


def edge_holds(c, L, res):
    """Does the case reach what it is named for?  (On the model's own head / size arrays.)"""
    e = c["edge"]
    head, size, act = res["_head"], res["_size"], res["_act"]
    if e[0] == "m":
        return L["m"] == e[1]
    if e[0] == "start":
        return bool(head[e[1]]) and int(size[e[1]]) == e[2] and (e[1] == 0 or not act[e[1] - 1] or bool(head[e[1]]))
    if e[0] == "span3":
        at, sz = e[1], e[2]
        t0, t1 = at // TILE, (at + sz - 1) // TILE
        return bool(head[at]) and int(size[at]) == sz and t1 - t0 >= 4 and not head[(t0 + 1) * TILE:t1 * TILE].any() and not act[at + sz]
    if e[0] == "active_at_most":
        return int(act.sum()) <= e[1] and L["m"] > 2 * TILE
    if e[0] == "groups":
        return int(res["counts"][1]) == e[1] and int(act.sum()) >= L["m"] - 1    # (k = 1: the last suffix is no longer than the key)
    if e[0] == "idle_tile":
        per = [int(act[t:t + TILE].sum()) for t in range(0, L["m"] - TILE + 1, TILE)]
        return 0 in per and TILE in per                    # a tile with nothing active, a tile with nothing finished
    if e[0] == "short":
        n, s, k = L["n"], L["sfx"], e[1]
        short = (n - s) <= k
        kc = L["keys"].astype(U64) & U64(L["kmask"])
        same_next = np.zeros(L["m"], bool)
        same_next[:-1] = kc[1:] == kc[:-1]
        # a short suffix whose successor shares its key (and is longer): both sides of the rule
        return bool((short & same_next).any()) and bool((~short[1:] & short[:-1] & same_next[:-1]).any())
    if e[0] == "payload":
        return bool(((L["keys"].astype(U64) & ~U64(L["kmask"])) != 0).any())
    return False


# ---- the forms ---------------------------------------------------------------------------------------------------------
FORM_TEXT_N = 65536 + 1025                                 # upper bits of the suffix number are in play


@functools.lru_cache(maxsize=None)
def form_text(n=FORM_TEXT_N, seed=21):
    """Four symbols, repeated phrases, ending in the lowest symbol."""
    T = phrase_text(n, seed)
    T[n - 5:] = 1
    return T


def init_forms(T):
    """name -> (list, the emit form that goes with it) for every initial form rank_step launches."""
    SA = sa_of(T)
    g = list_gram(T, SA, 8, 4, 9)
    gs = list_gram(T, SA, 8, 4, 9, split=True)
    levels = (0, 1, 2, 3, 4, 5, 6, 7, 7, 3, 1)
    return dict(u32=(list_sigma(T, SA, 8, wide=False), 2), u64=(list_sigma(T, SA, 8), 2), u64_payload=(list_sigma(T, SA, 8, payload_seed=4), 2),
                split=(list_sigma(T, SA, 8, split=True), 2), gram=(g, 3), gram_split=(gs, 3),
                levels=(with_levels(g, levels, g["long"]["chr_shift"] + 8), 3), levels_split=(with_levels(gs, levels, gs["long"]["chr_shift"] + 8), 3))


def list_code(T, SA, split, kbits=72):
    """Long items of the code form: codemodel.py's key words, second words and levels over T (which ends in its only zero
    byte) with the table built from T's own pair counts; an item's depth is its level's (code_level_depth), and that many
    characters its group really shares."""
    import codemodel as cm
    T = np.asarray(T, np.uint8)
    n = T.size
    lut, sigma = cm.lut_of(T, True)
    table, err = cm.build_table(cm.pair_counts(T, lut), sigma)
    assert err == 0
    mk = cm.make_keys(T, lut, table, kbits, split)
    hi_shift, chr_shift, lvl_shift = cm.key_layout(kbits, split)
    sfx = np.asarray(SA, np.int64)
    inv = np.zeros(256, np.uint8)
    present = np.flatnonzero(np.bincount(T, minlength=256))
    inv[lut[present[present > 0]]] = present[present > 0]
    return dict(n=n, m=n, init=True, wide=True, split=split, keys=mk["keys"][n - 1 - sfx], sfx=sfx, kmask=(1 << hi_shift) - 1, short_len=0,
                depth=np.array(LEVEL_DEPTH, np.int64)[mk["level"][sfx]], w=mk["w"][n - 1 - sfx], aglob=None, inv_lut=inv, claim="depth",
                long=dict(wmask=0xFFFFFFFF, hi_shift=hi_shift, chr_shift=chr_shift, chr_mask=0xFF, lvl_shift=lvl_shift, depth=0))


@functools.lru_cache(maxsize=None)
def code_text(n=30000, sigma=24, seed=4):
    """Structured text over `sigma` byte values (codemodel's generator) and the terminator: code keys of several levels."""
    import codemodel as cm
    return np.concatenate((cm.structured_text(np.random.default_rng(seed), n, sigma, False), np.zeros(1, np.uint8)))


def code_forms():
    T = code_text()
    SA = sa_of(T)
    return T, dict(code=(list_code(T, SA, False), 3), code_split=(list_code(T, SA, True), 3))


def claimed_depth(L, res):
    """What refined_breaks is asked about a step over L: one depth, the members' own (code form), or nothing."""
    return L["depth"][res["_act"]] if isinstance(L["claim"], str) else L["claim"]


def round_list(T, k, carry, wide=True):
    """The first round's list of T: the model's initial ranking (MODE 0) and its keys at depth k -> (list, rank[], h)."""
    L0 = list_sigma(T, sa_of(T), k, wide=wide)
    res = expect_pass(T, L0, 0, 2 if carry else 0)
    return next_round(T, L0, res, res["rank"], k, carry), res["rank"], k


def bytes_text(n, seed):
    """All 256 byte values, pairs repeated: a first round whose list carries every byte value as a character."""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 256, n, dtype=np.uint8)
    T[:512:2] = np.arange(256, dtype=np.uint8)             # every byte value precedes ...
    T[1:512:2] = 7                                         # ... a suffix that begins 7, x: tied with many under k = 1
    T[n - 2:] = 0
    return T


LF_CASES = ((1000, 0), (1000, 1), (1000, 2), (1000, 3), (300, 256), (800, 256), (3400, 256), (4097, 5))     # x = -, -, 500, 333, 1, 3, 13, 819


def emit_texts():
    """name -> T: suffix 0 finished at the last slot (out_n = n - 1: last_char) and suffix 0 still active."""
    tail = runs_text([50, 2100, 60])
    return dict(suffix0_last=np.concatenate((np.array([200], np.uint8), tail)), suffix0_active=runs_text(seam_lengths(K, 2047, 70)))


# ---- scan, scatter and key cases ---------------------------------------------------------------------------------------
SCAN_TILES = (1, 255, 256, 257, 4095, 4096, 4097, 8192, 8193)


def scan_inputs(nt, kind, seed=1):
    rng = np.random.default_rng(seed + nt)
    if kind == "zeros":
        return np.zeros(nt, np.uint32), np.zeros(nt, np.uint32), np.zeros(nt, np.uint32)
    if kind == "random":                                   # as reduce leaves them: counts up to 2048, head slots ascending with gaps (0: no head)
        c = (np.arange(nt, dtype=np.int64) * 2048 + rng.integers(1, 2049, nt)) * (rng.random(nt) < 0.6)
        return rng.integers(0, 2049, nt).astype(np.uint32), rng.integers(0, 1025, nt).astype(np.uint32), c.astype(np.uint32)
    if kind == "sum_max":                                  # the sums reach 2^32 - 1 exactly
        a = np.zeros(nt, np.int64)
        a[:] = (2 ** 32 - 1) // nt
        a[-1] += (2 ** 32 - 1) - int(a.sum())
        return a.astype(np.uint32), a[::-1].astype(np.uint32), np.zeros(nt, np.uint32)
    if kind == "max_first":                                # a max that lies only in the first entry
        c = np.zeros(nt, np.uint32)
        c[0] = 7
        return np.ones(nt, np.uint32), np.zeros(nt, np.uint32), c
    if kind == "max_part_end":                             # ... only in the last entry of a part (or of the array)
        c = np.zeros(nt, np.uint32)
        c[min(nt, SCAN_CHUNK) - 1] = 9
        return np.ones(nt, np.uint32), np.ones(nt, np.uint32), c
    raise ValueError(kind)


def scatter_case(chunks, last, n, bin_shift, one_bin, seed=2):
    """m = (chunks - 1) * 2048 + last distinct destinations below n; one_bin: all inside one bin of 2^bin_shift."""
    rng = np.random.default_rng(seed + chunks)
    m = (chunks - 1) * WIN_TILE + last
    if one_bin:
        assert m <= (1 << bin_shift) or bin_shift == 0
        where = rng.permutation(min(n, (1 << bin_shift) if bin_shift else n))[:m]
    else:
        where = np.sort(rng.permutation(n)[:m])
        for lo in range(0, m, 4096):                       # partitioned by the high bits, any order inside a window
            where[lo:lo + 4096] = rng.permutation(where[lo:lo + 4096])
    return where.astype(np.uint32), rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32)
