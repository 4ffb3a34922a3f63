"""The sorter's period rule, stated on its own (no GPU, no library): tests/runmodel.py for every period p >= 1.

T is the text as the sorter sees it; the end of T compares below every byte.  Position q is a break when q >= p and
T[q] != T[q - p]; k_p[s] = (the first break q >= s + p, or n) - s is the number of leading characters of suffix s that
are p-periodic (p = 1: the run length k[s]).  A list sorted to a depth h >= p holds, in every group, members with
k_p >= h only or none; those share their first p characters and so the same periodic string.  Their order: the falling
members (s + k reaches n, or T[s + k] < T[s + k - p]) first, by ascending k; the rising ones follow, by descending k;
members equal in that come from different stretches, share at least k characters and are ordered by rank[s + k].

  the period step  one round in which a member with k_p >= h takes the second key (type, k) or (type, n - k) instead of
                   rank[s + h] + 1; the list's depth h is not doubled by it (h_split = h).  Only valid once h >= p:
                   until then the rounds are ordinary ones
  later rounds     a member with k_p >= h_split looks up rank[s + max(h, k_p)], every other member rank[s + h]
  the gate         a list without a member with k_p > max(h, p) takes no period step
  the finder       neighbours of one group that lie d apart vote for d (votes())

The rule is right for every p: a wrong p costs rounds, never the order.  tests/test_periodmodel.py holds
sort_suffixes() to sorted() and to tests/runmodel.py."""

PERIOD_MAX = 4096


def period_lengths(T, p):
    """k_p[s] for every s, and the longest."""
    n = len(T)
    k = [0] * n
    nxt = n                                      # the first break at or behind x, for x = s + p
    for s in range(n - 1, -1, -1):
        x = s + p
        if x < n and T[x] != T[x - p]:
            nxt = x
        k[s] = nxt - s
    return k, max(k, default=0)


def falling(T, k, s, p):
    """The periodic stretch of s is followed by the end of T or by a byte below the one the period asks for."""
    e = s + k[s]
    return e >= len(T) or T[e] < T[e - p]


def period_key(T, k, s, p):
    """The period step's second key: one bit of type above a length."""
    n = len(T)
    return (0, k[s]) if falling(T, k, s, p) else (1, n - k[s])


def votes(T, depth):
    """The finder over the list sorted to `depth` characters (stable, positions descending inside a group): neighbours
    of one group that lie 2 <= d <= PERIOD_MAX apart vote for d.  -> {d: votes}."""
    T = bytes(T)
    n = len(T)
    order = sorted(range(n - 1, -1, -1), key=lambda s: T[s:s + depth])
    out = {}
    for a, b in zip(order, order[1:]):
        if T[a:a + depth] == T[b:b + depth]:
            d = abs(a - b)
            if 2 <= d <= PERIOD_MAX:
                out[d] = out.get(d, 0) + 1
    return out


def sort_suffixes(T, p=1, depth=1, step=True, others="lookup"):
    """Suffix order of T by prefix doubling from an initial ranking by `depth` characters.

    step: take the period step of period p at the first round whose depth h reaches p, if the gate lets it (a member
    with k_p > max(h, p)); others: what the members without a long stretch do in that round ("lookup": rank[s + h] as
    ever, "alone": they keep their group).
    Returns (order, rounds, stepped): stepped is the depth of the period step, or 0."""
    T = bytes(T)
    n = len(T)
    k, longest = period_lengths(T, p)
    order = sorted(range(n), key=lambda s: T[s:s + depth])
    rank = [0] * n

    def regroup(lo, hi, keys):
        """New ranks and groups for slots lo..hi, whose members are sorted by keys (same length as the slots)."""
        out, head = [], lo
        for j in range(lo, hi + 1):
            if j == hi or (j > lo and keys[j - lo] != keys[j - lo - 1]):
                if j - head > 1:
                    out.append((head, j))
                if j < hi:
                    head = j
            if j < hi:
                pending.append((order[j], head))
        return out

    pending = []
    groups = regroup(0, n, [T[s:s + depth] for s in order])
    for s, r in pending:
        rank[s] = r
    h, h_split, rounds = depth, 0, 0
    while groups:
        now = step and not h_split and h >= p and longest > max(h, p)
        pending, nxt = [], []
        for lo, hi in groups:
            keyed = []
            for s in order[lo:hi]:
                if now and k[s] >= h:
                    key = (1,) + period_key(T, k, s, p)
                elif now and others == "alone":
                    key = (0, 0, 0)
                else:
                    off = max(h, k[s]) if h_split and k[s] >= h_split else h
                    key = (0, 0, rank[s + off] + 1 if s + off < n else 0)
                keyed.append((key, s))
            keyed.sort()
            order[lo:hi] = [s for _, s in keyed]
            nxt += regroup(lo, hi, [q for q, _ in keyed])
        for s, r in pending:
            rank[s] = r
        groups = nxt
        rounds += 1
        if now:
            h_split = h
        else:
            h *= 2
        assert h <= 4 * n + 64, "the rounds do not end"
    return order, rounds, h_split


def period_lengths_np(T, p):
    """period_lengths() with numpy, for blocks of a megabyte: (k_p[] as uint32, the longest)."""
    import numpy as np
    T = np.asarray(T, np.uint8)
    n = T.size
    nb = np.full(n + 1, n, np.int64)             # nb[x]: the first break at or behind x
    if n > p:
        q = np.flatnonzero(T[p:] != T[:-p]) + p
        nb[q] = q
    nb = np.minimum.accumulate(nb[::-1])[::-1]
    s = np.arange(n, dtype=np.int64)
    k = nb[np.minimum(s + p, n)] - s
    return k.astype(np.uint32), int(k.max()) if n else 0
