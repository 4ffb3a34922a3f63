"""The sorter's long periods (BWTC_HIP_LONG_PERIODS=1), stated on their own (no GPU, no library).

tests/periodmodel.py states the period rule "for every p >= 1": k_p[], the step's keys, the gate and the rounds are its
functions, which take p as an argument and are used here as they are.  What that file limits to PERIOD_MAX = 4096 is the
finder alone; this file restates the finder for the distances 2 ... LONG_MAX = 2^24, and adds what the long periods bring
of their own: the finder's exact contract over a list, the wide probe's answer, k_p[] with both maxima, and the rounds a
block takes with a deferred step of period p.

  the finder  neighbours of one group (equal keys under kmask) that lie d apart, 2 <= d <= LONG_MAX, vote for d; with
              k1[] (the runs' lengths) a pair whose earlier member has k1 > d does not (two members of one run).  The
              candidates are the distances with `need` votes or more, most votes first, the smaller distance first among
              equals, at most CANDIDATES of them: candidates()
  the probe   is any of the windows [p + i span, p + (i + 1) span), those that end at or below n, free of breaks of
              period p?  probe()
  the rounds  a step of period p waits for the first doubling round whose depth reaches p: from a first round at depth d
              the depths are d, 2 d, 4 d ..., so ceil(log2(p / d)) rounds double before it (none when p <= d), the step is
              one more and the rounds behind it order what the stretches' tails leave: step_rounds() is the number that
              double before the step, and the GPU tests allow 3 more, the margin of tests/test_gpu_period_step.py.
              Without the step, suffixes s and s + p inside a stretch share k_p[s] - p characters and doubling needs a
              depth above that: plain_rounds() is the number of doublings from the first round's depth that pass the
              longest such tie, the "no step" rounds; the sorter's count lies at or above it and, by the same margin of
              3 (the first round, the rounds that order what the tails leave), at most 3 above: PLAIN_MARGIN."""
import math

import numpy as np

import periodmodel as pm

LONG_MAX = 1 << 24
CANDIDATES = 8
WORTH = 8                                        # kPeriodWorth
MIN_VOTES = 256                                  # kPeriodMinVotes
PLAIN_MARGIN = 3                                 # the sorter's rounds without the step: plain_rounds() ... plain_rounds() + 3


def need_of(n):
    """The votes that buy a period-length pass in a block of n bytes."""
    return max(MIN_VOTES, n // 64)


def vote_table(ks, vs, kmask, k1=None, dmax=LONG_MAX):
    """{distance: votes} over the list (ks[i], vs[i]) in list order."""
    ks = np.asarray(ks, np.uint64)
    vs = np.asarray(vs, np.uint32).astype(np.int64)
    if ks.size < 2:
        return {}
    same = ((ks[:-1] ^ ks[1:]) & np.uint64(kmask)) == 0
    d = np.abs(vs[:-1] - vs[1:])
    ok = same & (d >= 2) & (d <= dmax)
    if k1 is not None:
        first = np.minimum(vs[:-1], vs[1:])
        ok &= ~(np.asarray(k1, np.uint32).astype(np.int64)[first] > d)
    dist, count = np.unique(d[ok], return_counts=True)
    return {int(a): int(b) for a, b in zip(dist, count)}


def candidates(lst, kmask, need, k1=None, dmax=LONG_MAX):
    """The finder's contract over lst = (ks, vs): [(distance, votes)], exact, merged over short and long distances."""
    table = vote_table(lst[0], lst[1], kmask, k1, dmax)
    good = [(d, v) for d, v in table.items() if v >= need and v > 0]
    good.sort(key=lambda dv: (-dv[1], dv[0]))
    return good[:CANDIDATES]


def breaks_of(T, p):
    """One flag per position: q >= p and T[q] != T[q - p]."""
    T = np.asarray(T, np.uint8)
    b = np.zeros(T.size, bool)
    if T.size > p:
        b[p:] = T[p:] != T[:-p]
    return b


def probe(T, p, span):
    """The probe's answer (short or wide): an aligned window of `span` positions without a break."""
    n = len(T)
    if span <= 0 or n <= p + span:
        return False
    windows = (n - p) // span
    c = np.concatenate([[0], np.cumsum(breaks_of(T, p))])
    lo = p + span * np.arange(windows, dtype=np.int64)
    keep = lo + span <= n
    return bool(np.any(c[lo[keep] + span] == c[lo[keep]]))


def probe_span(p, h_first):
    """The window the sorter probes with: (W - p) / 2 for the worth W = 8 max(h_first, p)."""
    return (WORTH * max(h_first, p) - p) // 2


def lengths(T, p):
    """(k_p[] as uint32, the longest, the longest over the proper positions s: s + 1 < n and T[s] != T[s + 1])."""
    T = np.asarray(T, np.uint8)
    k, longest = pm.period_lengths_np(T, p)
    proper = 0
    if T.size >= 2:
        at = np.flatnonzero(T[:-1] != T[1:])
        proper = int(k[at].max()) if at.size else 0
    return k, longest, proper


def step_rounds(p, h_first):
    """The rounds that double before a step of period p, from a first round at depth h_first."""
    return max(0, math.ceil(math.log2(p / h_first))) if p > h_first else 0


def step_depth(p, h_first):
    """The depth the deferred step runs at: the first of h_first, 2 h_first, ... that reaches p."""
    return h_first << step_rounds(p, h_first)


def plain_rounds(T, p, h_first):
    """The "no step" rounds: the doublings h_first, 2 h_first, ... that pass the longest k_p - p."""
    tie = lengths(T, p)[1] - p
    return max(0, math.ceil(math.log2(tie / h_first))) if tie > h_first else 0


def takes_step(T, p, h_first, behind_run=False):
    """The schedule's rule for a voted long period: worth (g >= 8 max(h_first, p)) and the gate at the step's depth."""
    _, longest, proper = lengths(T, p)
    g = proper if behind_run else longest
    return 8 * p <= len(T) and g >= WORTH * max(h_first, p) and g > max(step_depth(p, h_first), p)


def sorted_list_np(T, depth=8):
    """sorted_list() for blocks of megabytes and depth <= 8 (a suffix shorter than that is padded with zeros: its votes
    are a handful): (ks, vs), the key being the `depth` characters as one number."""
    assert 1 <= depth <= 8
    T = np.asarray(T, np.uint8)
    n = T.size
    pad = np.concatenate([T, np.zeros(8, np.uint8)]).astype(np.uint64)
    key = np.zeros(n, np.uint64)
    for j in range(depth):
        key = (key << np.uint64(8)) | pad[j:j + n]
    order = np.argsort(key, kind="stable")
    return key[order], order.astype(np.uint32)


def window_order_list(T, depth=8):
    """sorted_list_np() with a group's members in another order than by position: by their suffix number's low 8 bits
    first, then by position, as a sort whose passes went by the suffix number leaves them.  Members of a stretch of
    period q that are neighbours there lie lcm(q, 256) apart, so the votes name a multiple of the period: the list the
    division is for (the hook-level case of tests/test_gpu_long_period_votes.py)."""
    ks, vs = sorted_list_np(T, depth)
    order = np.lexsort((vs, vs & np.uint32(255), ks))
    return ks[order], vs[order]


def divided(T, winner):
    """The division of a voted winner above the first round's depth (weigh_period): p / q for the winner's prime factors q,
    ascending, kept while the longest stretch stays as long; a factor that fails is not tried again.
    -> (the period left, the periods tried)."""
    g = lengths(T, winner)[1]
    p, rest, q, tried = winner, winner, 2, []
    while q <= rest and p // q >= 2:
        if rest % q:
            q += 1
            continue
        rest //= q
        tried.append(p // q)
        if lengths(T, p // q)[1] >= g:
            p //= q
        else:
            while rest % q == 0:
                rest //= q
    return p, tried


def sorted_list(T, depth):
    """The list sorted to `depth` characters as a stable sort leaves it (positions ascending inside a group): (ks, vs)
    with the group number as the key."""
    T = bytes(T)
    n = len(T)
    order = sorted(range(n), key=lambda s: T[s:s + depth])
    ks, g = [], 0
    for i, s in enumerate(order):
        if i and T[s:s + depth] != T[order[i - 1]:order[i - 1] + depth]:
            g += 1
        ks.append(g)
    return np.array(ks, np.uint64), np.array(order, np.uint32)
