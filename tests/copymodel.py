"""The sorter's rule for whole copies at places that are no period of the text between them (BWTC_HIP_COPIES=1), stated on
its own (no GPU, no library), on tests/runmodel.py's plain prefix-doubling sorter.

A list stands at a round of depth h: every tied group shares h characters, rank[] is complete and current -- a tied
suffix's rank is its group's head slot, a finished suffix's its own slot.
  F(G)   for a tied group G: every member s has s + 1 < n, and rank[s + 1] is one value for all members -- the successors
         of G lie in one group (which may be larger than G)
  P(s)   s is tied in this list and F(group(s)) holds; 0 for every other position
  K(s)   the number of consecutive positions q = s, s + 1, ... with P(q); 0 when P(s) is false
  the copy round   an ordinary doubling round in which member s looks up rank[s + K(s) + h] instead of rank[s + h] (key 0
         when s + K(s) + h >= n); the depth doubles as ever; K is made afresh from the groups of every round with a pass
  the gate         a pass is taken every round until one finds a longest K below its round's h (that round still looks up
         by its K); from then on the rounds are plain
Why it is right: P is a property of the group, and P(s) puts s + 1 and s' + 1 into one group, so by induction on the
position all members of a group have one K; for t <= K the suffixes s + t and s' + t lie in one group tied to depth h, so
the members share at least K + h characters and a look-up at K + h is a doubling look-up.  What a round leaves tied shares
K + 2h >= 2h characters.  sort_suffixes(check=True) asserts both statements in every round.

Runs and periods are not the rule's: in a run the member with k = h leaves the group, F fails and K is 0; back-to-back
copies of one piece are a period.

sort_suffixes_np() and copy_lengths_np() are the numpy twins, for blocks of a megabyte and the device's hook."""
import numpy as np

import mixedmodel


def copy_lengths(order, groups, rank, n):
    """order[slot]: the suffix at a slot; groups: (first slot, one past the last) of every tied group; rank[]: current.
    -> (K[s] for every s < n, the longest K)."""
    P = [0] * n
    for lo, hi in groups:
        members = order[lo:hi]
        if all(s + 1 < n for s in members) and len({rank[s + 1] for s in members}) == 1:
            for s in members:
                P[s] = 1
    K = [0] * n
    for s in range(n - 1, -1, -1):
        if P[s]:
            K[s] = (K[s + 1] if s + 1 < n else 0) + 1
    return K, max(K, default=0)


def _shared(T, members):
    """The characters all of `members` share (the end of T is a character of its own)."""
    n, a, c = len(T), members[0], 0
    while all(s + c < n for s in members) and all(T[s + c] == T[a + c] for s in members):
        c += 1
    return c


def sort_suffixes(T, depth=1, copies=True, gate=True, check=True):
    """Suffix order of T by prefix doubling from an initial ranking by `depth` characters; copies: with the rule; gate:
    with the gate (else a pass in every round).  -> (order, rounds, passes)."""
    T = bytes(T)
    n = len(T)
    order = sorted(range(n), key=lambda s: T[s:s + depth])
    rank = [0] * n

    def regroup(lo, hi, keys):
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
    h, rounds, passes, open_ = depth, 0, 0, copies
    while groups:
        K = None
        if open_:
            K, longest = copy_lengths(order, groups, rank, n)
            passes += 1
            if gate and longest < h:
                open_ = False
        pending, nxt = [], []
        for lo, hi in groups:
            members = order[lo:hi]
            if K is not None and check:
                assert len({K[s] for s in members}) == 1, (T, depth, h, members)
                assert _shared(T, members) >= K[members[0]] + h, (T, depth, h, members, K[members[0]])
            keyed = []
            for s in members:
                at = s + (K[s] if K is not None else 0) + h
                keyed.append((rank[at] + 1 if at < n else 0, s))
            keyed.sort()
            order[lo:hi] = [s for _, s in keyed]
            nxt += regroup(lo, hi, [q for q, _ in keyed])
        for s, r in pending:
            rank[s] = r
        groups = nxt
        rounds += 1
        h *= 2
        assert h <= 4 * n + 64, "the rounds do not end"
    return order, rounds, passes


# ---- the numpy twins ----------------------------------------------------------------------------

NONE = 0xFFFFFFFF                # "no successor": s + 1 = n


def tied_list_np(rank):
    """rank[] (a tied suffix's: its group's head slot) -> the list the device's pass is handed: (suffix, dense group
    number) of every tied suffix, in slot order."""
    rank = np.asarray(rank, np.int64)
    order = np.argsort(rank, kind="stable")
    r = rank[order]
    size = np.bincount(r, minlength=rank.size)[r]
    tied = size > 1
    suf, heads = order[tied], r[tied]
    new = np.ones(suf.size, bool)
    new[1:] = heads[1:] != heads[:-1]
    return suf.astype(np.uint32), (np.cumsum(new) - 1).astype(np.uint32)


def copy_lengths_np(suf, grp, rank, n):
    """The pass over a list -- suf[i], grp[i]: suffix and group number of entry i, a group's entries side by side -- and
    rank[0..n) -> (K[] as uint32, the longest K): copy_lengths() for lists of a megabyte."""
    suf, grp, rank = np.asarray(suf, np.int64), np.asarray(grp, np.int64), np.asarray(rank, np.int64)
    P = np.zeros(n, bool)
    if suf.size:
        v = np.where(suf + 1 < n, rank[np.minimum(suf + 1, n - 1)], -1)
        start = np.ones(suf.size, bool)
        start[1:] = grp[1:] != grp[:-1]
        at = np.flatnonzero(start)
        good = (np.minimum.reduceat(v, at) == np.maximum.reduceat(v, at)) & (np.minimum.reduceat(v, at) >= 0)
        P[suf[good[np.cumsum(start) - 1]]] = True
    stop = np.where(P, n, np.arange(n))                  # the first position at or behind q with P = 0
    stop = np.minimum.accumulate(stop[::-1])[::-1]
    K = (stop - np.arange(n)).astype(np.uint32)
    return K, int(K.max()) if n else 0


def sort_suffixes_np(T, depth=1, copies=True, gate=True):
    """sort_suffixes() with numpy -> (order, rounds, passes, entries): every round ranks the whole list, finished suffixes
    included -- the same refinement; the rounds counted are those with a tie left, entries is the sum of the tied over them."""
    T = np.asarray(T, np.uint8)
    n = T.size
    rank = mixedmodel._rank_by(T, depth, {})
    order = np.argsort(rank, kind="stable")
    h, rounds, passes, entries, open_ = depth, 0, 0, 0, copies
    while True:
        suf, grp = tied_list_np(rank)
        if not suf.size:
            return order, rounds, passes, entries
        K = 0
        if open_:
            K, longest = copy_lengths_np(suf, grp, rank, n)
            K = K.astype(np.int64)
            passes += 1
            if gate and longest < h:
                open_ = False
        rank, order, _ = mixedmodel._ranks(rank, mixedmodel._lookup(rank, K + h))
        entries += int(suf.size)
        rounds += 1
        h *= 2
        assert h <= 4 * n + 64, "the rounds do not end"
