"""The sorter's rule for a block with long runs AND stretches of a period p > 1 (BWTC_HIP_MIXED=1), stated on its own
(no GPU, no library), on tests/runmodel.py and tests/periodmodel.py.

A. A long run is a stretch of the period.  For a suffix s with k_1[s] >= p the positions s + p ... s + k_1 - 1 lie in
   the run with the positions p before them, so none is a p-break, and the run's end e = s + k_1 is one:
   T[e] != T[e - 1] = T[e - p].  Hence k_p[s] = k_1[s], and the type is the same: T[e] < T[e - p] is T[e] < T[e - 1].
   (statement_a() checks it position by position.)  A period step over k_p[] ranks every run longer than its depth as
   the run step would.
B. The period step asks that a group's members share h >= p characters and that rank[] is at least h deep -- not that
   the list is sorted to exactly h.  Both hold after a run step and ordinary rounds, so at the first round whose depth
   h reaches p, k_p[] takes the place of k_1[] and the period step runs with h_split = h.  A run member with k_1 >= p has
   k_p = k_1; one with k_1 < p <= h would look up at max(h, k_1) = h anyway.

The sequence, from an initial ranking by `depth` characters:
  p <= depth   one period step over k_p[] as the first round, if the longest PROPER stretch exceeds the depth; else the
               run step, if the longest run does
  p > depth    the run step as the first round, if the longest run exceeds the depth; rounds that look a member with
               k_1 >= h_split up at s + max(h, k_1); at the first round whose depth h reaches p, if the longest proper
               stretch exceeds max(h, p): k_p over k_1 and the period step; then rounds with k_p and the new h_split
The longest proper stretch is the largest k_p[s] over the s with s + 1 < n and T[s] != T[s + 1]: no position inside a run
of one byte, and one among any p consecutive positions of a stretch whose unit is not one byte over and over.

tests/test_mixedmodel.py holds sort_suffixes() to sorted(), to the two models it is built on, and to its numpy twin."""
import numpy as np

import periodmodel
import runmodel


def longest_proper(T, p):
    """The largest k_p[s] over the s with s + 1 < n and T[s] != T[s + 1] (0: there is none)."""
    k, _ = periodmodel.period_lengths(T, p)
    return max((k[s] for s in range(len(T) - 1) if T[s] != T[s + 1]), default=0)


def longest_proper_np(T, p, k=None):
    """longest_proper() with numpy, for blocks of a megabyte (k: period_lengths_np(T, p)[0], if it is at hand)."""
    T = np.asarray(T, np.uint8)
    if T.size < 2:
        return 0
    if k is None:
        k = periodmodel.period_lengths_np(T, p)[0]
    at = np.flatnonzero(T[:-1] != T[1:])
    return int(k[at].max()) if at.size else 0


def statement_a(T, p):
    """The positions s with k_1[s] >= p at which k_p[s] != k_1[s] or the types differ: none, by A."""
    k1, _ = runmodel.run_lengths(T)
    kp, _ = periodmodel.period_lengths(T, p)
    return [s for s in range(len(T)) if k1[s] >= p and
            (kp[s] != k1[s] or periodmodel.falling(T, kp, s, p) != runmodel.falling(T, k1, s))]


def plan(depth, p, longest_run, proper):
    """What the first round is: ("period", p), ("run", 1) or None."""
    if p >= 2 and p <= depth and proper > depth:
        return ("period", p)
    if longest_run > depth:
        return ("run", 1)
    return None


def sort_suffixes(T, p, depth=1):
    """Suffix order of T by prefix doubling from an initial ranking by `depth` characters, with the run step and the
    period step of period p >= 2 as the sequence above says.  -> (order, rounds, [(period, depth of its step), ...])."""
    T = bytes(T)
    n = len(T)
    k1, longest_run = runmodel.run_lengths(T)
    kp, _ = periodmodel.period_lengths(T, p)
    proper = longest_proper(T, p)
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
    first = plan(depth, p, longest_run, proper)
    period_left = first is None or first[0] == "run"     # a period step may still come
    k, pk, h, h_split, rounds, steps = k1, 1, depth, 0, 0, []
    while groups:
        now = False
        if rounds == 0 and first:
            now = True
            if first[0] == "period":
                k, pk = kp, p
        elif period_left and rounds > 0 and h >= p and proper > max(h, p):
            now, k, pk = True, kp, p
        if now and pk == p:
            period_left = False
        if h >= p and not now:
            period_left = period_left and proper > max(h, p)    # (the gate closes for good once the depth passes the stretch)
        pending, nxt = [], []
        for lo, hi in groups:
            keyed = []
            for s in order[lo:hi]:
                if now and k[s] >= h:
                    key = (1,) + periodmodel.period_key(T, k, s, pk)
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
            steps.append((pk, h))
        else:
            h *= 2
        assert h <= 4 * n + 64, "the rounds do not end"
    return order, rounds, steps


def one_step(T, p, depth=1):
    """The sorter with one step per block: the run step where the longest run exceeds the depth, else the period step.
    -> (order, rounds, [(period, depth)])."""
    _, longest_run = runmodel.run_lengths(T)
    if longest_run > depth:
        order, rounds, at = runmodel.sort_suffixes(T, depth)
        return order, rounds, [(1, at)] if at else []
    order, rounds, at = periodmodel.sort_suffixes(T, p, depth)
    return order, rounds, [(p, at)] if at else []


# ---- the numpy twin, for blocks of a megabyte ------------------------------------------------

def _ranks(keys_major, keys_minor):
    """rank[s] = the number of suffixes whose (major, minor) pair is smaller, and whether any two are equal."""
    order = np.lexsort((keys_minor, keys_major))
    a, b = keys_major[order], keys_minor[order]
    new = np.ones(order.size, bool)
    new[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
    head = np.maximum.accumulate(np.where(new, np.arange(order.size), 0))
    rank = np.empty(order.size, np.int64)
    rank[order] = head
    return rank, order, not new.all()


def _lookup(rank, off):
    """rank[s + off] + 1, or 0 past the end (off: one number or one per suffix)."""
    n = rank.size
    at = np.arange(n, dtype=np.int64) + off
    return np.where(at < n, rank[np.minimum(at, n - 1)] + 1, 0)


def _rank_by(T, d, memo):
    """The ranking of the suffixes by their first d characters."""
    if d not in memo:
        if d == 1:
            memo[d] = _ranks(T.astype(np.int64), np.zeros(T.size, np.int64))[0]
        else:
            a = d // 2
            memo[d] = _ranks(_rank_by(T, a, memo), _lookup(_rank_by(T, d - a, memo), a))[0]
    return memo[d]


def sort_suffixes_np(T, p, depth=1, mixed=True):
    """sort_suffixes() with numpy (mixed == False: one_step()'s sequence) -> (order, rounds, steps).  Every round ranks
    the whole list, finished suffixes included: the same refinement, and the rounds counted are those with a tie left."""
    T = np.asarray(T, np.uint8)
    n = T.size
    k1, longest_run = periodmodel.period_lengths_np(T, 1)
    kp, longest_p = periodmodel.period_lengths_np(T, p)
    k1, kp = k1.astype(np.int64), kp.astype(np.int64)
    proper = longest_proper_np(T, p, kp) if mixed else longest_p
    rank = _rank_by(T, depth, {})
    order = np.argsort(rank, kind="stable")
    tied = np.unique(rank).size < n
    first = plan(depth, p, longest_run, proper) if mixed else (("run", 1) if longest_run > depth else None)
    period_left = first is None or (mixed and first[0] == "run")
    k, pk, h, h_split, rounds, steps = k1, 1, depth, 0, 0, []
    s = np.arange(n, dtype=np.int64)
    while tied:
        now = False
        if rounds == 0 and first:
            now = True
            if first[0] == "period":
                k, pk = kp, p
        elif period_left and (rounds > 0 or first is None) and h >= p and proper > max(h, p):
            now, k, pk = True, kp, p
        if now and pk == p:
            period_left = False
        if h >= p and not now:
            period_left = period_left and proper > max(h, p)
        off = np.where(k >= h_split, np.maximum(h, k), h) if h_split else h
        key = _lookup(rank, off)
        if now:
            e = s + k
            fall = (e >= n) | (T[np.minimum(e, n - 1)] < T[np.minimum(e, n - 1) - pk])
            key = np.where(k >= h, (1 << 40) + np.where(fall, k, (1 << 36) + n - k), key)
        rank, order, tied = _ranks(rank, key)
        rounds += 1
        if now:
            h_split = h
            steps.append((pk, h))
        else:
            h *= 2
        assert h <= 4 * n + 64, "the rounds do not end"
    return order, rounds, steps
