"""The sorter's rule for a block with stretches of SEVERAL periods (BWTC_HIP_MULTI=1), stated on its own (no GPU, no
library), on tests/periodmodel.py and tests/mixedmodel.py.

A block's schedule is the run step (period 1) and up to three period steps.  From an initial ranking by `depth`
characters:
  p <= depth   a first-round step, if its gate exceeds the depth.  Several of them take consecutive rounds at that depth,
               the smallest period first; where one of them is a period step (p >= 2) the run step is dropped: that step
               ranks the runs too (statement A of tests/mixedmodel.py)
  p > depth    the entry waits for the first round whose depth h reaches p and runs there if its gate exceeds
               max(h, p); else it is dropped.  Two entries due at one depth take two consecutive rounds
The gate of period 1 is the longest run, the gate of a period p >= 2 its longest PROPER stretch (mixedmodel).  No step
doubles the depth.

The steps share ONE array of look-up lengths, K[s]: 0 until a step takes s.
  take     in the step of period p at depth h, member s is the step's when k_p[s] >= h and k_p[s] >= K[s].  It takes the
           closed-form key (type, k_p | n - k_p) with T[e - p], and K[s] = k_p[s]
  keep     everybody else takes the ordinary key at s + (K[s] ? max(h, K[s]) : h), in a step's own round too
Why the merge is right: the members of a tied group took the same closed-form key in every earlier step or none, so they
have one K and share K characters; k_p < K is then decided by characters they share, so all of them take or all keep
(check=True asserts both in every round, and that no look-up lies deeper than what the group shares).
merge=False is the overwrite form -- every step replaces K[] by its own lengths, 0 below its depth, which is what
BWTC_HIP_MIXED does with k_1[] -- kept so that tests can state what the merge buys.

On the device K[s] is one 32-bit word: the length in bits 0 ... 30, and bit 31 = "member of the current step", which
only the step's own round reads (merge_words()).

candidates() is the finder's answer over its vote table, accept() the host rule that turns candidates into entries.
tests/test_multimodel.py holds all of it to sorted(), to mixedmodel and to the numpy twin."""
import numpy as np

import mixedmodel
import periodmodel
from periodmodel import PERIOD_MAX

MAX_PERIOD_STEPS = 3
MAX_CANDIDATES = 8
WORTH = 8                       # a voted period's gate must reach this many times max(the first round's depth, p)
MEMBER = 1 << 31                # the merged word's flag: a member of the current step
LENGTH = MEMBER - 1


def gate_length(T, p):
    """The length a step's gate goes by: the longest run (p = 1), the longest proper stretch (p >= 2)."""
    return periodmodel.period_lengths(T, 1)[1] if p == 1 else mixedmodel.longest_proper(T, p)


def plan(depth, gates):
    """gates: {p: gate length} -> (the first-round steps' periods in their order, the waiting periods in theirs)."""
    first = sorted(p for p, g in gates.items() if p <= depth and g > depth)
    if any(p >= 2 for p in first):
        first = [p for p in first if p != 1]
    return first, sorted(p for p in gates if p > depth)


def _due(h, first, waiting, gates):
    """The period of this round's step, or 0; entries whose gate is shut at the depth that reaches them are dropped."""
    if first:
        return first.pop(0)
    while waiting and h >= waiting[0]:
        p = waiting.pop(0)
        if gates[p] > max(h, p):
            return p
    return 0


def merge_words(old, kp, h, fresh=False):
    """The merging stretch-length pass's stores: old words (ignored when fresh), the step's lengths k_p[], its depth h
    -> the words: k_p | MEMBER where the step takes s, else the old length (0: never taken)."""
    kp = np.asarray(kp, np.uint32)
    was = np.zeros(kp.size, np.uint32) if fresh else np.asarray(old, np.uint32) & np.uint32(LENGTH)
    take = (kp >= h) & (kp >= was)
    return np.where(take, kp | np.uint32(MEMBER), was).astype(np.uint32)


def _shared(T, members):
    """The characters all of `members` share (the end of T is a character of its own)."""
    n, a, c = len(T), members[0], 0
    while all(s + c < n for s in members) and all(T[s + c] == T[a + c] for s in members):
        c += 1
    return c


def sort_suffixes(T, periods, depth=1, merge=True, check=False, lengths=None):
    """Suffix order of T by prefix doubling from an initial ranking by `depth` characters, with the steps of `periods`
    (1: the run step) as the sequence above says.  lengths: {p: (k_p[], gate length)}, if they are at hand.
    -> (order, rounds, [(period, depth of its step), ...])."""
    T = bytes(T)
    n = len(T)
    periods = sorted(set(periods))
    assert sum(p >= 2 for p in periods) <= MAX_PERIOD_STEPS and all(1 <= p <= PERIOD_MAX for p in periods)
    if lengths is None:
        lengths = {p: (periodmodel.period_lengths(T, p)[0], gate_length(T, p)) for p in periods}
    gates = {p: lengths[p][1] for p in periods}
    first, waiting = plan(depth, gates)
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
    K, h, rounds, steps = [0] * n, depth, 0, []
    while groups:
        p = _due(h, first, waiting, gates)
        k = lengths[p][0] if p else None
        pending, nxt, took = [], [], []
        for lo, hi in groups:
            keyed, decided = [], set()
            for s in order[lo:hi]:
                mine = bool(p) and k[s] >= h and (k[s] >= K[s] or not merge)
                decided.add(mine)
                if mine:
                    off, key = 0, (1,) + periodmodel.period_key(T, k, s, p)
                    took.append(s)
                else:
                    off = max(h, K[s]) if K[s] else h
                    key = (0, 0, rank[s + off] + 1 if s + off < n else 0)
                keyed.append((key, s, off))
            if check:
                share = _shared(T, order[lo:hi])
                assert len(decided) == 1, (T, periods, depth, p, h, order[lo:hi])
                assert len({K[s] for s in order[lo:hi]}) == 1 and share >= h, (T, periods, depth, p, h, order[lo:hi])
                assert all(off <= share for _, _, off in keyed), (T, periods, depth, p, h, share, keyed)
            keyed.sort()
            order[lo:hi] = [s for _, s, _ in keyed]
            nxt += regroup(lo, hi, [q for q, _, _ in keyed])
        for s, r in pending:
            rank[s] = r
        if p and not merge:
            K = [x if x >= h else 0 for x in k]
        for s in took:
            K[s] = k[s]
        groups = nxt
        rounds += 1
        if p:
            steps.append((p, h))
        else:
            h *= 2
        assert h <= 4 * n + 64, "the rounds do not end"
    return order, rounds, steps


# ---- the numpy twin, for blocks of a megabyte ------------------------------------------------

def gate_length_np(T, p, k=None):
    if p == 1:
        return periodmodel.period_lengths_np(T, 1)[1]
    return mixedmodel.longest_proper_np(T, p, k)


def sort_suffixes_np(T, periods, depth=1, merge=True):
    """sort_suffixes() with numpy -> (order, rounds, steps).  Every round ranks the whole list, finished suffixes included:
    the same refinement, and the rounds counted are those with a tie left."""
    T = np.asarray(T, np.uint8)
    n = T.size
    periods = sorted(set(periods))
    assert sum(p >= 2 for p in periods) <= MAX_PERIOD_STEPS
    lengths = {p: periodmodel.period_lengths_np(T, p)[0].astype(np.int64) for p in periods}
    gates = {p: gate_length_np(T, p, lengths[p]) for p in periods}
    first, waiting = plan(depth, gates)
    rank = mixedmodel._rank_by(T, depth, {})
    order = np.argsort(rank, kind="stable")
    tied = np.unique(rank).size < n
    K, h, rounds, steps = np.zeros(n, np.int64), depth, 0, []
    s = np.arange(n, dtype=np.int64)
    while tied:
        p = _due(h, first, waiting, gates)
        key = mixedmodel._lookup(rank, np.where(K > 0, np.maximum(h, K), h))
        if p:
            k = lengths[p]
            mine = (k >= h) & ((k >= K) | (not merge))
            e = np.minimum(s + k, n - 1)
            fall = (s + k >= n) | (T[e] < T[e - p])
            key = np.where(mine, (1 << 40) + np.where(fall, k, (1 << 36) + n - k), key)
            K = np.where(mine, k, K) if merge else np.where(k >= h, k, 0)
        rank, order, tied = mixedmodel._ranks(rank, key)
        rounds += 1
        if p:
            steps.append((p, h))
        else:
            h *= 2
        assert h <= 4 * n + 64, "the rounds do not end"
    return order, rounds, steps


# ---- the finder's answer and the host's rule ---------------------------------------------------

def candidates(table, need):
    """table[d]: the votes for distance d, 0 ... PERIOD_MAX -> up to MAX_CANDIDATES (distance, votes) with a distance in
    2 ... PERIOD_MAX and votes >= need, by descending votes, the smaller distance first among equals."""
    table = np.asarray(table, np.int64)
    assert table.size == PERIOD_MAX + 1
    d = np.flatnonzero(table >= max(int(need), 1))
    d = d[d >= 2]
    d = d[np.lexsort((d, -table[d]))][:MAX_CANDIDATES]
    return [(int(x), int(table[x])) for x in d]


def accept(T, found, h_first):
    """The host's rule: candidates (distance, votes) in vote order -> the schedule's period entries [(p, gate, votes)],
    at most MAX_PERIOD_STEPS of them.  A candidate that is a multiple or a divisor of an accepted period is skipped (a
    p'-stretch longer than p is a p-stretch when p' divides p).  Each other one must be worth its pass -- its longest proper
    stretch g reaches WORTH x max(h_first, p) -- and a winner above h_first is divided by its prime factors while g stays
    as long.  (The device's probe refuses only what the worth test refuses: a stretch of the worth holds its window.)"""
    T = np.asarray(T, np.uint8)
    out = []
    for p, votes in found:
        if len(out) == MAX_PERIOD_STEPS:
            break
        if any(p % q == 0 or q % p == 0 for q, _, _ in out):
            continue
        g = mixedmodel.longest_proper_np(T, p)
        if g < WORTH * max(h_first, p):
            continue
        if p > h_first and g > p:
            rest, q = p, 2
            while q <= rest and p // q >= 2:
                if rest % q:
                    q += 1
                    continue
                rest //= q
                if mixedmodel.longest_proper_np(T, p // q) >= g:
                    p //= q
                else:
                    while rest % q == 0:
                        rest //= q
            g = mixedmodel.longest_proper_np(T, p)
            if any(p % q == 0 or q % p == 0 for q, _, _ in out):
                continue
        out.append((p, g, votes))
    return out
